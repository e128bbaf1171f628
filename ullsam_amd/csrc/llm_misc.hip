// HBM-bound kernels around the InternLM2 decoder stack.
#include "common.h"
#include "philox.h"

// ---- image-token scan (modeling_internvl_sam.py:135-139,194-199) -------------------------------------------------
// ids int64 [B,S] -> rank int32 [B,S] (k-th image token of the sample, or -1) and range int32 [B,2] = [min_idx, max_idx+1)
__global__ __launch_bounds__(64) void scan_image_tokens_kernel(const long long* __restrict__ ids, int* __restrict__ rank,
                                                               int* __restrict__ range, int S, long long img_id) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int count = 0, lo = S, hi = -1;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool is_img = s < S && ids[(long)b * S + s] == img_id;
        const unsigned long long m = __ballot(is_img);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (s < S) rank[(long)b * S + s] = is_img ? count + before : -1;
        if (is_img) { lo = min(lo, s); hi = max(hi, s); }
        count += __popcll(m);
    }
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
    if (lane == 0) { range[2 * b] = lo; range[2 * b + 1] = hi + 1; }
}

// ---- token embedding gather + image-token scatter (modeling_internvl_sam.py:124-158 / :412-429) -----------------
// out f32 [B*S, D]: row <- table[id] or, where rank >= 0, vit_embeds[b, rank % n_img]   (the "repeat" branch :143-145)
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const T* __restrict__ table, const long long* __restrict__ ids,
                                                           const int* __restrict__ rank, const float* __restrict__ vit, float* __restrict__ out,
                                                           long rows, int S, int D, int n_img, long vocab) {
    const int dq = D / 4;
    const long total = rows * dq;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / dq;
        const int c = (int)(i - r * dq) * 4;
        const int rk = rank ? rank[r] : -1;
        float4 v;
        if (rk >= 0 && vit) {
            const long b = r / S;
            v = *reinterpret_cast<const float4*>(vit + ((long)b * n_img + (rk % n_img)) * D + c);
        } else {
            long long id = ids[r];
            if (id < 0) id = 0;
            if (id >= vocab) id = vocab - 1;
            v = load4(table + id * D + c);
        }
        *reinterpret_cast<float4*>(out + r * D + c) = v;
    }
}

extern "C" int ullsam_scan_image_tokens(const long long* ids, int* rank, int* range, int B, int S, long long img_id, void* stream) {
    if (B == 0) return 0;
    scan_image_tokens_kernel<<<B, 64, 0, reinterpret_cast<hipStream_t>(stream)>>>(ids, rank, range, S, img_id);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_embed_tokens(int dtype, const void* table, const long long* ids, const int* rank, const float* vit_embeds,
                                   float* out, int B, int S, int D, int n_img, long vocab, void* stream) {
    ULLSAM_CHECK(D % 4 == 0, "embed_tokens: D %% 4 != 0");
    const long rows = (long)B * S;
    if (rows == 0) return 0;
    const long total = rows * (D / 4);
    const int grid = (int)min((total + 255) / 256, (long)2048 * 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == 0) embed_tokens_kernel<float><<<grid, 256, 0, s>>>((const float*)table, ids, rank, vit_embeds, out, rows, S, D, n_img, vocab);
    else embed_tokens_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)table, ids, rank, vit_embeds, out, rows, S, D, n_img, vocab);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ---- rows [start_b, start_b + n) of each sample (hidden_states[-1][:, start:end], modeling_internvl_sam.py:198-200) ----
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, const int* __restrict__ range,
                                                          int B, int S, int n, int rq) {  // rq = 16-byte chunks per row
    const long total = (long)B * n * rq;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long t = i;
        const int c = t % rq; t /= rq;
        const int r = t % n; t /= n;
        const int b = (int)t;
        int src = range[2 * b] + r;
        if (src >= S) src = S - 1;
        if (src < 0) src = 0;
        out[i] = in[((long)b * S + src) * rq + c];
    }
}

extern "C" int ullsam_gather_rows(const void* in, void* out, const int* range, int B, int S, int n, int row_bytes, void* stream) {
    ULLSAM_CHECK(row_bytes % 16 == 0, "gather_rows: row_bytes %% 16 != 0");
    const long total = (long)B * n * (row_bytes / 16);
    if (total == 0) return 0;
    const int grid = (int)min((total + 255) / 256, (long)2048 * 8);
    gather_rows_kernel<<<grid, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>((const uint4*)in, (uint4*)out, range, B, S, n, row_bytes / 16);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ---- wqkv de-interleave + RoPE + KV-cache append (modeling_internlm2.py:361-388, rotate_half :233-247) -----------
// qkv T [B*S, KVH*(G+2)*hd] with per-token layout (kv_head, [q x G, k, v], hd)
// q_out T [B*S, H*hd] (head = kv_head*G + g), k_cache/v_cache T [B, KVH, cap, hd] written at cache_pos0 + s
// pos int32 [B,S] -> rows of the fp32 cos/sin tables [n_pos, hd] (cat(freqs,freqs) layout, :166-170)
template <typename T>
__global__ __launch_bounds__(256) void rope_split_kernel(const T* __restrict__ qkv, T* __restrict__ q_out, T* __restrict__ k_cache,
                                                         T* __restrict__ v_cache, const int* __restrict__ pos, const float* __restrict__ cosT,
                                                         const float* __restrict__ sinT, int B, int S, int KVH, int G, int hd, int cap,
                                                         int cache_pos0, int tab_rows) {
    const int half = hd / 2, hq = half / 4;
    const int gs = G + 2;
    const long total = (long)B * S * KVH * gs * hq;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long t = i;
        const int d4 = (int)(t % hq) * 4; t /= hq;
        const int g = t % gs; t /= gs;
        const int kv = t % KVH; t /= KVH;
        const long tok = t;  // b*S + s
        const int b = (int)(tok / S), s = (int)(tok % S);
        const T* src = qkv + tok * ((long)KVH * gs * hd) + ((long)kv * gs + g) * hd;
        const float4 x1 = load4(src + d4), x2 = load4(src + half + d4);
        if (g == gs - 1) {  // value: no rotation
            T* dst = v_cache + (((long)b * KVH + kv) * cap + cache_pos0 + s) * hd;
            store4(dst + d4, x1);
            store4(dst + half + d4, x2);
            continue;
        }
        const int p = min(max(pos[tok], 0), tab_rows - 1);  // never read outside the tables (the reference would raise IndexError)
        const float4 c1 = *reinterpret_cast<const float4*>(cosT + (long)p * hd + d4);
        const float4 c2 = *reinterpret_cast<const float4*>(cosT + (long)p * hd + half + d4);
        const float4 s1 = *reinterpret_cast<const float4*>(sinT + (long)p * hd + d4);
        const float4 s2 = *reinterpret_cast<const float4*>(sinT + (long)p * hd + half + d4);
        // q_embed = q*cos + rotate_half(q)*sin, rotate_half = cat(-x2, x1)
        const float4 o1 = make_float4(x1.x * c1.x - x2.x * s1.x, x1.y * c1.y - x2.y * s1.y, x1.z * c1.z - x2.z * s1.z, x1.w * c1.w - x2.w * s1.w);
        const float4 o2 = make_float4(x2.x * c2.x + x1.x * s2.x, x2.y * c2.y + x1.y * s2.y, x2.z * c2.z + x1.z * s2.z, x2.w * c2.w + x1.w * s2.w);
        T* dst;
        if (g == gs - 2) dst = k_cache + (((long)b * KVH + kv) * cap + cache_pos0 + s) * hd;
        else dst = q_out + tok * ((long)KVH * G * hd) + ((long)kv * G + g) * hd;
        store4(dst + d4, o1);
        store4(dst + half + d4, o2);
    }
}

extern "C" int ullsam_rope_split(int dtype, const void* qkv, void* q_out, void* k_cache, void* v_cache, const int* pos,
                                 const float* cos_tab, const float* sin_tab, int B, int S, int KVH, int G, int hd, int cap,
                                 int cache_pos0, int tab_rows, void* stream) {
    ULLSAM_CHECK(hd % 8 == 0, "rope_split: hd %% 8 != 0");
    ULLSAM_CHECK(tab_rows > 0, "rope_split: empty cos/sin tables");
    ULLSAM_CHECK(cache_pos0 + S <= cap, "rope_split: cache overflow (%d + %d > %d)", cache_pos0, S, cap);
    const long total = (long)B * S * KVH * (G + 2) * (hd / 8);
    if (total == 0) return 0;
    const int grid = (int)min((total + 255) / 256, (long)2048 * 8);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == 0) rope_split_kernel<float><<<grid, 256, 0, s>>>((const float*)qkv, (float*)q_out, (float*)k_cache, (float*)v_cache, pos, cos_tab, sin_tab, B, S, KVH, G, hd, cap, cache_pos0, tab_rows);
    else rope_split_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)qkv, (bf16*)q_out, (bf16*)k_cache, (bf16*)v_cache, pos, cos_tab, sin_tab, B, S, KVH, G, hd, cap, cache_pos0, tab_rows);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ---- greedy argmax over fp32 logits [R, V] -> int64 (first maximum wins, like torch.argmax) ---------------------
__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ x, long long* __restrict__ out, long V, long ld) {
    __shared__ float sv[16];
    __shared__ long long si[16];
    const float* row = x + (long)blockIdx.x * ld;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float best = -INFINITY;
    long long bi = tid;   // the thread's first index: a row of nothing but -inf (or NaN, which `>` never takes) yields index 0 like torch.argmax, never an index outside [0, V)
    // four independent loads per trip; within a thread indices increase, so `>` keeps the first maximum
    for (long i0 = tid; i0 < V; i0 += 4096) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (i0 + 1024 * u < V) ? row[i0 + 1024 * u] : -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v[u] > best) { best = v[u]; bi = i0 + 1024 * u; }
    }
    auto better = [](float v, long long j, float w, long long k) { return v > w || (v == w && j < k); };
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(best, o, 64);
        const long long j = __shfl_xor(bi, o, 64);
        if (better(v, j, best, bi)) { best = v; bi = j; }
    }
    if (lane == 0) { sv[wv] = best; si[wv] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (better(sv[w], si[w], best, bi)) { best = sv[w]; bi = si[w]; }
        out[blockIdx.x] = bi;
    }
}

extern "C" int ullsam_argmax(const float* logits, long long* out, int rows, long V, long ld, void* stream) {
    if (rows == 0) return 0;
    argmax_kernel<<<rows, 1024, 0, reinterpret_cast<hipStream_t>(stream)>>>(logits, out, V, ld);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

// ---- seeded top-k / top-p sampling on fp32 logits [R, V] -> int64 (app.py:469-477: chat(do_sample, T 0.7, top_k 50, top_p 0.9)) ----
// One 1024-thread workgroup per row:
//   1. V > 1024: the smallest of the 1024 threads' maxima is a floor -- at least 1024 >= top_k values lie at or above it, so nothing below it is a
//      candidate and the histograms below count only what is left (a few percent of an ordinary row);
//   2. radix select of the k-th largest order-preserving key, 8 bits a pass (integer LDS histogram), ended as soon as everything at or above the
//      selected bin fits the 1024 sort slots;
//   3. those values into the slots (key << 32 | ~id), bitonic sort descending = (value descending, id ascending): the first min(top_k, V) are the
//      candidates.  Only when more than 1024 values would remain after all four passes (ties at the k-th value) are the tied ones taken in id order
//      by a scan over contiguous per-thread ranges;
//   4. wave 0: softmax over the candidates, nucleus prefix, draw.
// Integer atomics only and a total order in the sort: the result is a pure function of (row, T, k, p, seed, step).
__device__ __forceinline__ unsigned int sample_key(float x) {   // larger value <=> larger key; NaN -> -inf, -0 -> +0 (equal values, equal keys)
    unsigned int b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) b = 0xff800000u;
    if ((b << 1) == 0u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sample_value(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Philox4x32-10 (philox.h), word 0 of the block with counter (step lo, step hi, 0, 0) and key (seed lo, seed hi)
__device__ __forceinline__ unsigned int philox4x32_10_word0(unsigned long long seed, unsigned long long step) {
    return philox4x32_10_word0((unsigned int)seed, (unsigned int)(seed >> 32), (unsigned int)step, (unsigned int)(step >> 32), 0u, 0u);
}

template <typename T> __device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

#define SAMPLE_CAP 1024
__global__ __launch_bounds__(1024) void sample_topk_topp_kernel(const float* __restrict__ x, long long* __restrict__ out, long V, long ld, float temperature,
                                                                int top_k, float top_p, const unsigned long long* __restrict__ seeds, unsigned long long step,
                                                                const float* __restrict__ u_in, float* __restrict__ u_out, long long* __restrict__ cand_ids,
                                                                float* __restrict__ cand_p) {
    __shared__ unsigned long long cand[SAMPLE_CAP];   // key << 32 | (2^32 - 1 - id); 0 = empty (below every key: -inf's is 0x007fffff)
    __shared__ float sp[SAMPLE_CAP];
    __shared__ int hist[256];
    __shared__ unsigned int wred[16];
    __shared__ int s_above, s_inbin, s_digit, s_n;
    __shared__ float s_total;
    const long r = blockIdx.x;
    const float* row = x + r * ld;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int kk = (int)min((long)top_k, V);
    cand[tid] = 0ull;
    if (tid == 0) s_n = 0;
    unsigned int prefix = 0u, mask = 0u, floor_key = 0u;
    int above = 0, inbin = (int)min(V, (long)SAMPLE_CAP);
    if (V > SAMPLE_CAP) {
        unsigned int tmax = 0u;
        for (long i0 = tid; i0 < V; i0 += 4096) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (i0 + 1024 * u < V) ? row[i0 + 1024 * u] : -INFINITY;
#pragma unroll
            for (int u = 0; u < 4; ++u) tmax = max(tmax, sample_key(v[u]));   // (a slot past V counts as -inf, the smallest key: it never raises a maximum)
        }
        for (int o = 32; o > 0; o >>= 1) tmax = min(tmax, (unsigned int)__shfl_xor(tmax, o, 64));
        if (lane == 0) wred[wv] = tmax;
        __syncthreads();
        floor_key = wred[0];
        for (int w = 1; w < 16; ++w) floor_key = min(floor_key, wred[w]);
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (long i0 = tid; i0 < V; i0 += 4096) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = (i0 + 1024 * u < V) ? row[i0 + 1024 * u] : 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned int k = sample_key(v[u]);
                    if (i0 + 1024 * u < V && k >= floor_key && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
                }
            }
            __syncthreads();
            if (wv == 0) {   // bins from the top: lane l owns 255 - 4l .. 252 - 4l; the bin in which the count from above reaches kk
                int h[4], s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = hist[255 - 4 * lane - j]; s += h[j]; }
                int a = above + wave_scan_incl(s, lane) - s;
                if (a < kk && kk <= a + s) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (a < kk && kk <= a + h[j]) { s_above = a; s_inbin = h[j]; s_digit = 255 - 4 * lane - j; }
                        a += h[j];
                    }
                }
            }
            __syncthreads();
            above = s_above; inbin = s_inbin;
            prefix |= (unsigned int)s_digit << shift;
            mask |= 255u << shift;
            if (above + inbin <= SAMPLE_CAP) break;
        }
    } else {
        __syncthreads();
    }
    // more than the slots hold at or above the k-th key after all 32 bits: the surplus are values EQUAL to the k-th (above < kk <= 1024)
    const bool tied = above + inbin > SAMPLE_CAP;
    for (long i0 = tid; i0 < V; i0 += 4096) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (i0 + 1024 * u < V) ? row[i0 + 1024 * u] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long i = i0 + 1024 * u;
            const unsigned int k = sample_key(v[u]);
            if (i < V && (tied ? k > prefix : (k >= floor_key && (k & mask) >= prefix))) {
                const int slot = atomicAdd(&s_n, 1);
                if (slot < SAMPLE_CAP) cand[slot] = ((unsigned long long)k << 32) | (0xffffffffu - (unsigned int)i);
            }
        }
    }
    __syncthreads();
    int n = min(s_n, SAMPLE_CAP);
    if (tied) {   // the kk - above lowest ids among the values equal to the k-th: thread t scans ids [t C, (t + 1) C), ranks by an exclusive scan of the threads' counts
        const int need = kk - above;
        const long C = (V + 1023) / 1024, lo = min(V, tid * C), hi = min(V, lo + C);
        int cnt = 0;
        for (long i = lo; i < hi && cnt < need; ++i) cnt += sample_key(row[i]) == prefix;   // (clamped at need: ranks below need are exact, later threads see >= need)
        const int incl = wave_scan_incl(cnt, lane);
        if (lane == 63) hist[wv] = incl;
        __syncthreads();
        int rank = incl - cnt;
        for (int w = 0; w < wv; ++w) rank += hist[w];
        for (long i = lo; i < hi && rank < need; ++i)
            if (sample_key(row[i]) == prefix) { cand[above + rank] = ((unsigned long long)prefix << 32) | (0xffffffffu - (unsigned int)i); ++rank; }
        n = kk;
        __syncthreads();
    }
    int P = 64;
    while (P < n) P <<= 1;
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int p = tid ^ j;
            if (tid < P && p > tid) {
                const unsigned long long a = cand[tid], b = cand[p];
                if (((tid & k2) == 0) ? a < b : a > b) { cand[tid] = b; cand[p] = a; }
            }
            __syncthreads();
        }
    if (wv == 0) {   // ---- wave 0: lane l owns candidates [l C, (l + 1) C), and reads back only the sp[] slots it wrote ----
        const int C = (kk + 63) / 64, j0 = min(kk, lane * C), j1 = min(kk, j0 + C);
        const float x0 = sample_value((unsigned int)(cand[0] >> 32));
        const bool degenerate = x0 == INFINITY || x0 == -INFINITY;   // a +inf (the first one leads the order) or nothing above -inf (id 0 leads): all mass on candidate 0
        float u;
        if (u_in) u = u_in[r];
        else u = (float)(philox4x32_10_word0(seeds[r], step) >> 8) * 5.9604644775390625e-8f;   // 2^-24: [0, 1)
        if (lane == 0 && u_out) u_out[r] = u;
        float ls = 0.f;
        for (int j = j0; j < j1; ++j) {
            const float e = degenerate ? (j == 0 ? 1.f : 0.f) : expf((sample_value((unsigned int)(cand[j] >> 32)) - x0) / temperature);
            sp[j] = e;
            ls += e;
        }
        const float sum = wave_sum(ls);
        float lp = 0.f;
        for (int j = j0; j < j1; ++j) { const float p = sp[j] / sum; sp[j] = p; lp += p; }
        // nucleus: candidate j stays iff j == 0 or the mass before it is below top_p; the kept set is the prefix in front of the first one that goes
        float m = wave_scan_incl(lp, lane) - lp;
        int first_out = kk;
        for (int j = j0; j < j1; ++j) {
            if (first_out == kk && j != 0 && top_p < 1.f && !(m < top_p)) first_out = j;
            m += sp[j];
        }
        for (int o = 32; o > 0; o >>= 1) first_out = min(first_out, __shfl_xor(first_out, o, 64));
        const int K = first_out;
        float lt = 0.f;
        for (int j = j0; j < min(j1, K); ++j) lt += sp[j];
        const float incl = wave_scan_incl(lt, lane);
        const float total = __shfl(incl, 63, 64);
        // draw: the first kept candidate (of non-zero probability) whose inclusive mass exceeds u * total, else the last such candidate
        const float target = u * total;
        float c = incl - lt;
        int pick = kk, last = 0;
        for (int j = j0; j < min(j1, K); ++j) {
            c += sp[j];
            if (sp[j] > 0.f) {
                last = j;
                if (pick == kk && c > target) pick = j;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            pick = min(pick, __shfl_xor(pick, o, 64));
            last = max(last, __shfl_xor(last, o, 64));
        }
        if (pick == kk) pick = last;
        if (lane == 0) { out[r] = (long long)(0xffffffffu - (unsigned int)cand[pick]); s_above = K; s_total = total; }
    }
    __syncthreads();
    const int K = s_above;
    const float total = s_total;
    if (cand_ids)
        for (int j = tid; j < top_k; j += 1024) cand_ids[r * top_k + j] = j < kk ? (long long)(0xffffffffu - (unsigned int)cand[j]) : -1ll;
    if (cand_p)
        for (int j = tid; j < top_k; j += 1024) cand_p[r * top_k + j] = j < K ? sp[j] / total : 0.f;
}

extern "C" int ullsam_sample_topk_topp(const float* logits, long long* out, int rows, long V, long ld, float temperature, int top_k, float top_p,
                                       const unsigned long long* seeds, unsigned long long step, const float* u_in, float* u_out,
                                       long long* cand_ids, float* cand_p, void* stream) {
    ULLSAM_CHECK(top_k >= 1 && top_k <= SAMPLE_CAP, "sample_topk_topp: top_k %d outside 1..%d", top_k, SAMPLE_CAP);
    ULLSAM_CHECK(temperature > 0.f, "sample_topk_topp: temperature must be > 0");
    ULLSAM_CHECK(top_p > 0.f, "sample_topk_topp: top_p must be > 0");
    ULLSAM_CHECK(rows >= 0 && V >= 1 && V <= 0x7fffffffL && ld >= V, "sample_topk_topp: rows %d, V %ld, ld %ld", rows, V, ld);
    ULLSAM_CHECK(seeds || u_in, "sample_topk_topp: neither seeds nor u_in");
    if (rows == 0) return 0;
    sample_topk_topp_kernel<<<rows, 1024, 0, reinterpret_cast<hipStream_t>(stream)>>>(logits, out, V, ld, temperature, top_k, top_p, seeds, step, u_in, u_out,
                                                                                       cand_ids, cand_p);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
