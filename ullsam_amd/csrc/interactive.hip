// The interactive loop's display tail (app.py:283-287 postprocess_mask, 635-645 upsample + threshold, 692-707 save_instance's canvas write,
// 748-772 visualize_masks, 807-820 export_mask's un-pad) as ONE pass over the display image: from the low-resolution logits of P masks to the
// binary masks, the painted label canvas, the blended overlay and area + box per mask.  No frame-sized intermediate is written.
// Definitions: DESIGN.md "7b, continued: the interactive loop"; host form: utils/interactive.py click_finish_host.
//
// Per display pixel (y, x) of [H, W], which lies at (top + y, left + x) of the padded square of side `side`:
//   frame pixel   fy = min(((2 (y + top) + 1) S) / (2 side), S - 1), fx likewise (Image.NEAREST of the S x S frame to side x side, 64-bit integers)
//   logit         v_p = the bilinear value of low[p] at (fy, fx) of its [LH, LW] -> [S, S] resize: tap_of / lerp_rn of common.h, the arithmetic of
//                 resize_bilinear_kernel (decoder.hip), so the same bits
//   mask          m_p = v_p > thr
//   canvas        paint: id = first_id + p of the LAST p with m_p, else the id the canvas holds
//   overlay       c = image[y, x]; id > 0: c[k] = lut_inst[(id - 1) % K][k][c[k]]; highlight and m_{P-1}: c[k] = lut_cur[k][c[k]]
//   stats[p]      area, x0, y0, x1, y1 of m_p (inclusive maxima, an empty mask -> zeros)
//
// Work split: a block of 4 waves owns a 256-pixel column strip of CF_ROWS consecutive rows; a lane owns one column, so its column tap is
// computed once and the row tap is wave-uniform.  P is the inner loop: the P low-resolution maps (256 KB each at SAM's size) are re-read from
// cache by neighbouring lanes and rows.  Statistics: a ballot per (row, p) gives the wave's count and column extent; each wave accumulates
// into its own LDS slots (no LDS atomics), wave 0 adds the block's four slots and issues integer atomics on `scratch` (only for masks the
// block saw), then takes a ticket; the block that draws the last ticket decodes scratch into stats with plain stores.
#include "common.h"

#define CF_ROWS 4          // rows per block
#define CF_MAX_P 512       // 4 waves x P x 5 ints of LDS (40 KB at the cap)
#define CF_PAINT 1
#define CF_HIGHLIGHT 2

struct CfGeom {
    int P, LH, LW, S, H, W, side, top, left, first_id, flags, K;
    float thr;
};

__device__ __forceinline__ int cf_frame_index(int d, int off, int S, int side) {
    return (int)min(((2L * ((long)d + off) + 1) * S) / (2L * side), (long)S - 1);
}

// scratch i32 [5 P + 1], zeroed by the launcher: per mask {area, max(W - x), max(H - y), max(x + 1), max(y + 1)} over its pixels, then the ticket
// counter.  Every field grows from zero, so an untouched row decodes to the empty mask.
__global__ __launch_bounds__(256) void click_finish_kernel(const float* __restrict__ low, CfGeom g, const unsigned char* __restrict__ image,
                                                            int* __restrict__ canvas, const unsigned char* __restrict__ lut_inst,
                                                            const unsigned char* __restrict__ lut_cur, unsigned char* __restrict__ mask,
                                                            unsigned char* __restrict__ overlay, int* __restrict__ stats, int* __restrict__ scratch) {
    extern __shared__ int cf_acc[];                       // [4 waves][P][5], used only when stats != NULL
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = g.P;
    if (stats) {
        for (int i = threadIdx.x; i < 4 * P * 5; i += 256) cf_acc[i] = 0;
        __syncthreads();
    }
    int* acc = cf_acc + wave * P * 5;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const bool in_x = x < g.W;
    const int xc = min(x, g.W - 1);                       // a lane past the right edge computes the last column and writes nothing
    const float sy = (float)g.LH / (float)g.S, sx = (float)g.LW / (float)g.S;
    const Tap tx = tap_of(cf_frame_index(xc, g.left, g.S, g.side), sx, g.LW);
    const long plane = (long)g.LH * g.LW, per = (long)g.H * g.W;
    const int y_end = min((int)(blockIdx.y + 1) * CF_ROWS, g.H);
    const int wave_x0 = blockIdx.x * 256 + wave * 64;
    for (int y = blockIdx.y * CF_ROWS; y < y_end; ++y) {
        const Tap ty = tap_of(cf_frame_index(y, g.top, g.S, g.side), sy, g.LH);
        const long pix = (long)y * g.W + xc;
        int id = canvas ? canvas[pix] : 0;
        const int id_in = id;
        bool m = false;
        const float* r0 = low + (long)ty.i0 * g.LW;
        const float* r1 = low + (long)ty.i1 * g.LW;
        for (int p = 0; p < P; ++p, r0 += plane, r1 += plane) {
            const float a = lerp_rn(r0[tx.i0], r0[tx.i1], tx.l);
            const float b = lerp_rn(r1[tx.i0], r1[tx.i1], tx.l);
            m = in_x && lerp_rn(a, b, ty.l) > g.thr;
            if (mask && in_x) mask[p * per + pix] = m ? 1 : 0;
            if (m && (g.flags & CF_PAINT)) id = g.first_id + p;
            if (stats) {
                const unsigned long long bal = __ballot(m);
                if (bal && lane == 0) {                   // wave-uniform values, one lane updates the wave's own slots
                    int* s = acc + p * 5;
                    const int xl = wave_x0 + __builtin_ctzll(bal), xh = wave_x0 + 63 - __builtin_clzll(bal);
                    s[0] += __builtin_popcountll(bal);
                    s[1] = max(s[1], g.W - xl);
                    s[2] = max(s[2], g.H - y);
                    s[3] = max(s[3], xh + 1);
                    s[4] = max(s[4], y + 1);
                }
            }
        }
        if (!in_x) continue;
        if (canvas && id != id_in) canvas[pix] = id;
        if (overlay) {
            unsigned char c0 = image[pix * 3], c1 = image[pix * 3 + 1], c2 = image[pix * 3 + 2];
            if (id > 0) {
                const unsigned char* t = lut_inst + (long)((id - 1) % g.K) * 768;
                c0 = t[c0]; c1 = t[256 + c1]; c2 = t[512 + c2];
            }
            if (m && (g.flags & CF_HIGHLIGHT)) {          // m is m_{P-1} after the loop
                c0 = lut_cur[c0]; c1 = lut_cur[256 + c1]; c2 = lut_cur[512 + c2];
            }
            overlay[pix * 3] = c0; overlay[pix * 3 + 1] = c1; overlay[pix * 3 + 2] = c2;
        }
    }
    if (!stats) return;
    __syncthreads();
    if (wave != 0) return;
    // wave 0: the block's sums -> scratch (integer atomics, agent scope), then the ticket.  One wave issues both, in order; the release makes
    // the atomics visible before the ticket, the last block's acquire orders its reads after every other block's ticket.
    for (int p = lane; p < P; p += 64) {
        const int *s0 = cf_acc + p * 5, *s1 = s0 + P * 5, *s2 = s1 + P * 5, *s3 = s2 + P * 5;
        const int area = s0[0] + s1[0] + s2[0] + s3[0];
        if (area) {
            int* d = scratch + p * 5;
            atomicAdd(d, area);
#pragma unroll
            for (int k = 1; k < 5; ++k) atomicMax(d + k, max(max(s0[k], s1[k]), max(s2[k], s3[k])));
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the atomics above have been performed before the ticket is taken
    int ticket = 0;
    if (lane == 0) ticket = __hip_atomic_fetch_add(scratch + 5 * P, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __shfl(ticket, 0, 64);
    if (ticket != (int)(gridDim.x * gridDim.y) - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int p = lane; p < P; p += 64) {
        int v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = __hip_atomic_load(scratch + p * 5 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int* o = stats + p * 5;
        const bool any = v[0] > 0;
        o[0] = v[0];
        o[1] = any ? g.W - v[1] : 0;
        o[2] = any ? g.H - v[2] : 0;
        o[3] = any ? v[3] - 1 : 0;
        o[4] = any ? v[4] - 1 : 0;
    }
}

// low f32 [P, LH, LW]; image u8 [H, W, 3] (nullable unless overlay); canvas i32 [H, W] (nullable; read for the overlay, written where painted);
// lut_inst u8 [K, 3, 256], lut_cur u8 [3, 256] (nullable unless overlay); outputs, each nullable: mask u8 [P, H, W], overlay u8 [H, W, 3],
// stats i32 [P, 5] with scratch i32 [5 P + 1].  flags: 1 = paint, 2 = highlight.
extern "C" int ullsam_click_finish(const float* low, int P, int LH, int LW, int S, int H, int W, int side, int top, int left, float thr,
                                   const unsigned char* image, int* canvas, int first_id, int flags, const unsigned char* lut_inst, int K,
                                   const unsigned char* lut_cur, unsigned char* mask, unsigned char* overlay, int* stats, int* scratch,
                                   void* stream) {
    ULLSAM_CHECK(low && P >= 1 && P <= CF_MAX_P && LH > 0 && LW > 0 && S > 0 && H > 0 && W > 0 && side > 0,
                 "click_finish: need low, 1 <= P <= 512 and positive sizes");
    ULLSAM_CHECK((long)H * W < (1L << 31) / 3 && (long)LH * LW * P < (1L << 31) && H <= 65535 * CF_ROWS,
                 "click_finish: H * W * 3 and P * LH * LW must stay below 2^31, H below 2^18");
    ULLSAM_CHECK(top >= 0 && left >= 0 && (long)top + H <= side && (long)left + W <= side, "click_finish: the window (top, left, H, W) must lie inside the square of side `side`");
    ULLSAM_CHECK((flags & ~(CF_PAINT | CF_HIGHLIGHT)) == 0, "click_finish: unknown flag");
    ULLSAM_CHECK(!overlay || (image && lut_inst && lut_cur && K >= 1), "click_finish: an overlay needs the image, both blend tables and K >= 1");
    ULLSAM_CHECK(!(flags & CF_PAINT) || canvas, "click_finish: paint needs a canvas");
    ULLSAM_CHECK(!stats || scratch, "click_finish: stats need scratch i32 [5 P + 1]");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (stats && hipMemsetAsync(scratch, 0, (size_t)(5 * P + 1) * 4, s) != hipSuccess) {
        ullsam_set_error("click_finish: memset failed");
        return -2;
    }
    CfGeom g{P, LH, LW, S, H, W, side, top, left, first_id, flags, K > 0 ? K : 1, thr};
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)((H + CF_ROWS - 1) / CF_ROWS));
    const size_t lds = stats ? (size_t)4 * P * 5 * 4 : 0;
    click_finish_kernel<<<grid, 256, lds, s>>>(low, g, image, canvas, lut_inst, lut_cur, mask, overlay, stats, scratch);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
