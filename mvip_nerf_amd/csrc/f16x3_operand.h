// The operand format of the split-precision ("f16x3") contractions -- 3x3 convolution, plain GEMM, attention and the
// GroupNorm / LayerNorm / GEGLU producers that feed them -- and the ONLY home of the decisions it rests on:
//   * the scale rule: a tensor is multiplied by s = 2^k before it is split, k = clamp(10 - e, -60, 60) with
//     frexpf(absmax, &e), so that absmax * s lies in [2^9, 2^10) and the lo terms stay in fp16's normal range;
//     s = 1 when the maximum is 0 or not a usable number.  A scale travels as scale2 = {s, 1/s};
//   * the absolute-maximum filter: NaN, inf and anything not below 3.0e38 is ignored, not propagated;
//   * the split: v -> hi = fp16(v), lo = fp16(v - hi), eight values = one 16-byte hi and one 16-byte lo fragment.
// Everything here is __forceinline__ (or a kernel with internal linkage): the callers' instruction streams are what they
// were when each of them wrote these out by hand.
#pragma once
#include "common.h"

namespace mvip {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// 16 bytes per lane, global memory -> LDS by DMA (no register staging); dst_wave is the wave's 1-KiB piece
__device__ __forceinline__ void glds16b(const void *src_lane, void *dst_wave) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src_lane,
                                     (__attribute__((address_space(3))) void *)dst_wave, 16, 0, 0);
}

// eight (already scaled) floats -> their hi and lo fp16 fragments
__device__ __forceinline__ void split8(const float (&v)[8], uint4 &hi, uint4 &lo) {
    unsigned h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h16x2 a, b;
        a.x = (_Float16)v[2 * i]; a.y = (_Float16)v[2 * i + 1];
        b.x = (_Float16)(v[2 * i] - (float)a.x); b.y = (_Float16)(v[2 * i + 1] - (float)a.y);
        h[i] = __builtin_bit_cast(unsigned, a); l[i] = __builtin_bit_cast(unsigned, b);
    }
    hi = make_uint4(h[0], h[1], h[2], h[3]);
    lo = make_uint4(l[0], l[1], l[2], l[3]);
}

// *lo_flag |= 1 when a lo fragment of a packed weight image holds a non-zero half (tail word 12 of the image; looked at
// before the atomic: once set, nobody writes again)
__device__ __forceinline__ void note_lo(const uint4 &lo, unsigned *lo_flag) {
    if (((lo.x | lo.y | lo.z | lo.w) & 0x7fff7fffu) && *reinterpret_cast<volatile unsigned *>(lo_flag) == 0u) atomicOr(lo_flag, 1u);
}

// ---- absolute maximum --------------------------------------------------------------------------------
constexpr float ABSMAX_LIMIT = 3.0e38f;              // maxima at or above it (inf included) do not count

// the running maximum m after looking at v
__device__ __forceinline__ float absmax_take(float m, float v) {
    v = fabsf(v);
    return (v == v && v < ABSMAX_LIMIT) ? fmaxf(m, v) : m;
}

// maximum over the 64 lanes, in every lane
__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}

// maximum over a 256-thread workgroup: the xor tree inside each wave, then the four waves through LDS (one barrier).
// Every thread must call it; thread 0 is the one that uses the result.
__device__ __forceinline__ float block256_max(float m) {
    m = wave_max(m);
    __shared__ float wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

// ---- the scale rule ----------------------------------------------------------------------------------
__host__ __device__ __forceinline__ float scale_for_absmax(float absmax) {
    float s = 1.f;
    if (absmax > 0.f && absmax < ABSMAX_LIMIT) {
        int e;
        frexpf(absmax, &e);
        int k = 10 - e;
        k = k > 60 ? 60 : (k < -60 ? -60 : k);
        s = ldexpf(1.f, k);
    }
    return s;
}

// scale2 = {s, 1/s} for a tensor whose absolute maximum is absmax
__device__ __forceinline__ void store_scale2(float *scale2, float absmax) {
    const float s = scale_for_absmax(absmax);
    scale2[0] = s;
    scale2[1] = 1.f / s;
}

// scale2 from the maximum collected (atomicMax on float bits) in *bits; *bits is left ZERO for its next user (the scratch
// word is owned by the caller and travels zero between calls, which saves a zeroing launch per use)
static __global__ void scale_from_bits_kernel(float *__restrict__ scale2, unsigned *__restrict__ bits) {
    const float m = __uint_as_float(*bits);
    *bits = 0u;
    store_scale2(scale2, m);
}

// ---- launches shared by the translation units, each defined once (csrc/f16x3_producers.hip, csrc/conv3x3.hip) ----
// *bits (zero on entry) <- bits of the absolute maximum of x[0..n), then scale2 <- its scale; *bits keeps the maximum.
// n == 0 launches the scale alone.
void launch_absmax_then_scale(const float *x, int64_t n, unsigned *bits, float *scale2, hipStream_t st);
// the same in ONE launch: words2 are two caller-owned scratch words, zero on entry and left zero (n > 0)
void launch_absmax_scale(const float *x, int64_t n, unsigned *words2, float *scale2, hipStream_t st);
// y = (sum_s partial[s]) / (s_w s_x) + bias + chan_add + residual over `rows` rows (sample, output row) of HW values,
// the splits of a split-K launch added in index order; bias has `M` entries (row % M)
void launch_split_reduce(const float *partial, int splits, int64_t rows, int M, int64_t HW, const float *w_scale2,
                         const float *x_scale2, const float *bias, const float *chan_add, const float *residual, float *y,
                         hipStream_t st);

// 32-row tiles per workgroup of the convolution and the 32/64-row GEMM kernels: the largest MT dividing rows/32 whose grid
// still has two workgroups per CU (else 1); 0 when the rows are no multiple of 32
static inline int cv_mt(int64_t Cout, int64_t tiles) {
    if (Cout % 32 != 0) return 0;
    const int64_t rows = Cout / 32;
    for (int mt = 2; mt > 1; mt >>= 1)                 // MT = 4 (one workgroup per CU) measured slower than two MT = 2
        if (rows % mt == 0 && tiles * (rows / mt) >= 512) return mt;
    return 1;
}

}  // namespace mvip
