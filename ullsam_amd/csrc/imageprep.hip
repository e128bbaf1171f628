// Image preprocessing: Pillow's antialiased 8-bit resize (Resample.c, 8 bits per channel) as two integer passes, and the app's min-max
// normalisation to uint8 (DESIGN.md "7b, continued (image preprocessing)").
//
// The coefficient and bounds tables come from the host (ops.aa_tables: float64, rounded to 22-bit fixed point exactly as Pillow does); the
// device does only the integer work, so both passes are bit-exact by construction:
//   out = clamp((2^21 + sum_t src[xmin + t] * k[t]) >> 22, 0, 255)   (signed 32-bit sum, arithmetic shift)
// The horizontal pass rounds to uint8 into a [rows, OW, C] buffer; the vertical pass reads it.  A pass that Pillow skips (out == in) gets the
// identity table (one tap of 2^22), which copies.
#include "common.h"
#include "ullsam_hip.h"

#define IP_BITS 22

__device__ __forceinline__ unsigned char ip_clip8(int acc) {
    const int v = (acc + (1 << (IP_BITS - 1))) >> IP_BITS;
    return (unsigned char)min(max(v, 0), 255);
}

// ---- horizontal pass ------------------------------------------------------------------------------------------------------------------
// One thread per output pixel (all C channels).  The source is addressed by three strides (interleaved [H, W, C]: (W C, C, 1); planar
// [C, H, W]: (W, 1, H W)) and sits at (top, left) of a virtual VH x VW image that is zero elsewhere: virtual rows row0 .. row0 + rows - 1 are
// computed, row r going to tmp[(r - row0), :, :].  bounds i32 [OW, 2] = (xmin, n); coef i32 [ksize, OW] (tap-major: lanes read neighbours).
// grid (ceil(OW / 256), min(rows, 65535)), block 256.
template <int C>
__global__ __launch_bounds__(256) void resize_aa_h_kernel(const unsigned char* __restrict__ src, long s_row, long s_col, long s_chan, int IH,
                                                          int IW, int top, int left, int row0, int rows, const int* __restrict__ bounds,
                                                          const int* __restrict__ coef, int OW, unsigned char* __restrict__ tmp) {
    const int xx = blockIdx.x * 256 + threadIdx.x;
    if (xx >= OW) return;
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const int t0 = max(left - xmin, 0), t1 = min(left + IW - xmin, n);      // the taps that fall on real columns
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const int y = row0 + r - top;                                       // real source row
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0;
        if (y >= 0 && y < IH) {
            const unsigned char* p = src + (long)y * s_row + (long)(xmin + t0 - left) * s_col;
            for (int t = t0; t < t1; ++t, p += s_col) {
                const int k = coef[(long)t * OW + xx];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += (int)p[c * s_chan] * k;
            }
        }
        unsigned char* o = tmp + ((long)r * OW + xx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = ip_clip8(acc[c]);
    }
}

// ---- vertical pass + epilogue ---------------------------------------------------------------------------------------------------------
// One thread per output pixel (all C channels); a block is one row segment, so bounds and coefficients are uniform over the block.
// tmp u8 [rows, OW, C] holds virtual rows row0 ..; bounds i32 [OH, 2] = (ymin, n) with row0 <= ymin, ymin + n <= row0 + rows; coef i32
// [OH, ksize].  out_u8 [OH, OW, C] and / or out_f32: planes c = 0..2 at c * f_plane + y * f_row + x, value lut[c * 256 + v] (C == 1: the
// one channel through each plane's table; C == 4: the fourth channel has no plane).  grid (ceil(OW / 256), min(OH, 65535)), block 256.
template <int C>
__global__ __launch_bounds__(256) void resize_aa_v_kernel(const unsigned char* __restrict__ tmp, int row0, int OW, const int* __restrict__ bounds,
                                                          const int* __restrict__ coef, int ksize, int OH, unsigned char* __restrict__ out_u8,
                                                          const float* __restrict__ lut, float* __restrict__ out_f32, long f_plane, long f_row) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= OW) return;
    const long row_b = (long)OW * C;
    for (int y = blockIdx.y; y < OH; y += gridDim.y) {
        const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
        const int* k = coef + (long)y * ksize;
        const unsigned char* p = tmp + (long)(ymin - row0) * row_b + (long)x * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0;
        for (int t = 0; t < n; ++t, p += row_b) {
            const int kt = k[t];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[c] * kt;
        }
        unsigned char v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = ip_clip8(acc[c]);
        if (out_u8) {
            unsigned char* o = out_u8 + (long)y * row_b + (long)x * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = v[c];
        }
        if (out_f32) {
            float* o = out_f32 + (long)y * f_row + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c * f_plane] = lut[c * 256 + v[C == 1 ? 0 : c]];
        }
    }
}

// ---- min-max normalisation to uint8 ---------------------------------------------------------------------------------------------------
// mm u32 [2] = (min, max) as order-preserving keys: the value itself for uint16; for float32 the bits with the sign bit flipped
// (non-negative) or all bits flipped (negative), so unsigned order is numeric order.  Integer atomics: any arrival order gives the same bits.
__device__ __forceinline__ unsigned ip_key(unsigned short v) { return v; }
__device__ __forceinline__ unsigned ip_key(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ip_unkey(unsigned k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ void minmax_init_kernel(unsigned* mm) {
    mm[0] = 0xffffffffu;
    mm[1] = 0u;
}

template <typename T>
__global__ __launch_bounds__(256) void minmax_kernel(const T* __restrict__ x, long n, unsigned* __restrict__ mm) {
    __shared__ unsigned s_lo[4], s_hi[4];
    unsigned lo = 0xffffffffu, hi = 0u;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const unsigned k = ip_key(x[i]);
        lo = min(lo, k);
        hi = max(hi, k);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o, 64));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(mm, min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3])));
        atomicMax(mm + 1, max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3])));
    }
}

// ((img - img.min()) / (img.max() - img.min() + 1e-8) * 255).astype(np.uint8) as numpy evaluates it for a uint16 array: the difference in
// uint16, the quotient and the product in float64, truncation.
__global__ __launch_bounds__(256) void normalize_u16_kernel(const unsigned short* __restrict__ x, long n, const unsigned* __restrict__ mm,
                                                            unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    const unsigned lo = mm[0];
    const double den = (double)(unsigned short)(mm[1] - lo) + 1e-8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = (unsigned char)(int)((double)(unsigned short)(x[i] - lo) / den * 255.0);
}

// ... and for a float32 array: every step in float32 (1e-8 rounded to float32 first).  The quotient goes through float64: the double
// quotient of two floats rounded to float is the correctly rounded float quotient (53 >= 2 * 24 + 2), whatever the device's `/` expands to.
__global__ __launch_bounds__(256) void normalize_f32_kernel(const float* __restrict__ x, long n, const unsigned* __restrict__ mm,
                                                            unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    const float lo = ip_unkey(mm[0]), hi = ip_unkey(mm[1]);
    const float den = (hi - lo) + 1e-8f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float d = x[i] - lo;
        const float q = (float)((double)d / (double)den);
        out[i] = (unsigned char)(int)(q * 255.0f);
    }
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
static unsigned ip_blocks(long n) { return (unsigned)max(1L, min((n + 255) / 256, 2048L)); }

extern "C" int ullsam_resize_u8_aa_h(const unsigned char* src, long s_row, long s_col, long s_chan, int IH, int IW, int C, int top, int left,
                                     int VH, int VW, int row0, int rows, const int* bounds, const int* coef, int ksize, int OW,
                                     unsigned char* tmp, void* stream) {
    ULLSAM_CHECK(C == 1 || C == 3 || C == 4, "resize_u8_aa_h: C must be 1, 3 or 4");
    ULLSAM_CHECK(IH > 0 && IW > 0 && OW > 0 && ksize > 0 && s_row >= 0 && s_col >= 0 && s_chan >= 0, "resize_u8_aa_h: need IH, IW, OW, ksize > 0 and strides >= 0");
    ULLSAM_CHECK(top >= 0 && left >= 0 && (long)top + IH <= VH && (long)left + IW <= VW, "resize_u8_aa_h: the image must lie inside the [VH, VW] window");
    ULLSAM_CHECK(row0 >= 0 && rows >= 0 && (long)row0 + rows <= VH, "resize_u8_aa_h: rows row0 .. row0 + rows must lie inside [0, VH)");
    if (rows == 0) return 0;
    const dim3 grid((unsigned)((OW + 255) / 256), (unsigned)min(rows, 65535));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define IP_H(CC) resize_aa_h_kernel<CC><<<grid, 256, 0, s>>>(src, s_row, s_col, s_chan, IH, IW, top, left, row0, rows, bounds, coef, OW, tmp)
    if (C == 1) IP_H(1); else if (C == 3) IP_H(3); else IP_H(4);
#undef IP_H
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int ullsam_resize_u8_aa_v(const unsigned char* tmp, int row0, int rows, int OW, int C, const int* bounds, const int* coef, int ksize,
                                     int OH, unsigned char* out_u8, const float* lut, float* out_f32, long f_plane, long f_row, void* stream) {
    ULLSAM_CHECK(C == 1 || C == 3 || C == 4, "resize_u8_aa_v: C must be 1, 3 or 4");
    ULLSAM_CHECK(rows > 0 && OW > 0 && OH > 0 && ksize > 0 && row0 >= 0, "resize_u8_aa_v: need rows, OW, OH, ksize > 0 and row0 >= 0");
    ULLSAM_CHECK(out_u8 || out_f32, "resize_u8_aa_v: no output asked for");
    ULLSAM_CHECK(!out_f32 || (lut && f_row >= OW && f_plane >= 0), "resize_u8_aa_v: the float output needs its table and f_row >= OW");
    const dim3 grid((unsigned)((OW + 255) / 256), (unsigned)min(OH, 65535));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define IP_V(CC) resize_aa_v_kernel<CC><<<grid, 256, 0, s>>>(tmp, row0, OW, bounds, coef, ksize, OH, out_u8, lut, out_f32, f_plane, f_row)
    if (C == 1) IP_V(1); else if (C == 3) IP_V(3); else IP_V(4);
#undef IP_V
    ULLSAM_LAUNCH_CHECK();
    return 0;
}

template <typename T> static int ip_minmax(const T* x, long n, unsigned* mm, void* stream, const char* what) {
    ULLSAM_CHECK(n > 0, "%s: need n > 0", what);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    minmax_init_kernel<<<1, 1, 0, s>>>(mm);
    ULLSAM_LAUNCH_CHECK();
    minmax_kernel<T><<<ip_blocks(n), 256, 0, s>>>(x, n, mm);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
extern "C" int ullsam_minmax_u16(const unsigned short* x, long n, unsigned* mm, void* stream) { return ip_minmax(x, n, mm, stream, "minmax_u16"); }
extern "C" int ullsam_minmax_f32(const float* x, long n, unsigned* mm, void* stream) { return ip_minmax(x, n, mm, stream, "minmax_f32"); }

extern "C" int ullsam_normalize_to_u8_u16(const unsigned short* x, long n, const unsigned* mm, unsigned char* out, void* stream) {
    ULLSAM_CHECK(n > 0, "normalize_to_u8_u16: need n > 0");
    normalize_u16_kernel<<<ip_blocks(n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(x, n, mm, out);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
extern "C" int ullsam_normalize_to_u8_f32(const float* x, long n, const unsigned* mm, unsigned char* out, void* stream) {
    ULLSAM_CHECK(n > 0, "normalize_to_u8_f32: need n > 0");
    normalize_f32_kernel<<<ip_blocks(n), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(x, n, mm, out);
    ULLSAM_LAUNCH_CHECK();
    return 0;
}
