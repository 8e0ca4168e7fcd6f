// Producers of the split-precision ("f16x3") operands (csrc/f16x3_operand.h): the absolute maximum of a tensor and its
// power-of-two scale, and the writers of "split planes" xs[n][C/16][kg 2][hl 2][pixels][8 halves] -- the B operand of the 3x3
// convolution (csrc/conv3x3.hip), of the plain GEMM (csrc/gemm_f16x3.hip) and the Q / K operands of attention -- from fp32
// tensors: plain, strided, 2x up-sampled, GroupNorm(+SiLU)-applied, or gathered as im2col columns (with col2im for the
// data gradient of the layers that run as a GEMM).
#include "f16x3_operand.h"
#include <stdlib.h>

namespace mvip {

// ---- power-of-two scale from the absolute maximum ----------------------------------------------------
__global__ void __launch_bounds__(256) cv_absmax_kernel(const float *__restrict__ x, int64_t n, unsigned *__restrict__ out) {
    float m = 0.f;
    auto take = [&](float v) { m = absmax_take(m, v); };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        const int64_t n4 = n >> 2;
        // four independent 16-byte loads per thread and trip: one in flight per thread (2 MB over the whole grid) held this
        // streaming read to ~1 TB/s
        int64_t i = tid;
        for (; i + 3 * stride < n4; i += 4 * stride) {
            const float4 a = x4[i], b = x4[i + stride], c = x4[i + 2 * stride], d = x4[i + 3 * stride];
            take(a.x); take(a.y); take(a.z); take(a.w); take(b.x); take(b.y); take(b.z); take(b.w);
            take(c.x); take(c.y); take(c.z); take(c.w); take(d.x); take(d.y); take(d.z); take(d.w);
        }
        for (; i < n4; i += stride) { const float4 v = x4[i]; take(v.x); take(v.y); take(v.z); take(v.w); }
        for (int64_t k = (n4 << 2) + tid; k < n; k += stride) take(x[k]);
    } else {
        for (int64_t i = tid; i < n; i += stride) take(x[i]);
    }
    m = block256_max(m);                    // one atomic per workgroup: same-address atomics serialise (~10 ns each)
    if (threadIdx.x == 0) atomicMax(out, __float_as_uint(m));
}

// One-launch form: the maxima are collected in words[0] (zero on entry), every workgroup takes a ticket in words[1]
// (zero on entry) and the LAST one turns the maximum into scale2 = {s, 1/s} and leaves both words zero again.  The two
// words are caller-owned scratch that travels zero between calls on a stream (saves the zeroing and the scale launch).
__global__ void __launch_bounds__(256) cv_absmax_scale_kernel(const float *__restrict__ x, int64_t n, unsigned *__restrict__ words,
                                                             float *__restrict__ scale2) {
    float m = 0.f;
    auto take = [&](float v) { m = absmax_take(m, v); };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        const int64_t n4 = n >> 2;
        int64_t i = tid;                               // eight independent 16-byte loads per thread and trip: these launches are
        for (; i + 7 * stride < n4; i += 8 * stride) { // latency-bound (a trip is one memory round trip), see absmax_blocks
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = x4[i + u * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) { take(v[u].x); take(v[u].y); take(v[u].z); take(v[u].w); }
        }
        for (; i < n4; i += stride) { const float4 v = x4[i]; take(v.x); take(v.y); take(v.z); take(v.w); }
        for (int64_t k = (n4 << 2) + tid; k < n; k += stride) take(x[k]);
    } else {
        for (int64_t i = tid; i < n; i += stride) take(x[i]);
    }
    m = block256_max(m);
    if (threadIdx.x == 0) {
        atomicMax(words, __float_as_uint(m));
        __threadfence();
        const unsigned ticket = atomicAdd(words + 1, 1u);
        if (ticket == gridDim.x - 1) {
            const float mx = __uint_as_float(atomicExch(words, 0u));         // every workgroup's maximum has landed
            atomicExch(words + 1, 0u);
            store_scale2(scale2, mx);
        }
    }
}

// one workgroup per 64 K elements, at most one per CU: every workgroup ends with two atomics on the same pair of words,
// which serialise in L2 (512 workgroups: 1.54 ms over the 94 calls of an SDS step, 256: see profiles)
static inline unsigned absmax_blocks(int64_t n) {
    // Small tensors are latency-bound (a trip of a thread's loop is one memory round trip, a workgroup's two atomics serialise
    // in L2): 64 floats per thread on at most 64 workgroups; large ones are bandwidth-bound: 64 K floats per workgroup on at
    // most 256.  Per launch inside a graph replay (tools/absmax_sweep.py, profiles/r4_absmax_sweep.json): 0.16 M floats 6.2 ->
    // 3.7 us, 0.66 M 6.5 -> 4.1, 2.6 M 6.7 -> 5.9, 33 M 25.2 (unchanged).  MVIP_ABSMAX_FPT / MVIP_ABSMAX_MAXB override (tuning).
    const char *ef = getenv("MVIP_ABSMAX_FPT"), *eb = getenv("MVIP_ABSMAX_MAXB");
    if (ef || eb) {
        const int64_t fpt = ef ? atoi(ef) : 256, maxb = eb ? atoi(eb) : 256;
        const int64_t b = (n + 256 * fpt - 1) / (256 * fpt);
        return (unsigned)(b < 1 ? 1 : (b > maxb ? maxb : b));
    }
    int64_t b = (n + 256 * 64 - 1) / (256 * 64);
    if (b > 64) {
        const int64_t big = (n + 256 * 256 - 1) / (256 * 256);
        b = big > 64 ? big : 64;
    }
    return (unsigned)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

// scale2 from the maximum collected in *bits, which KEEPS it (the packed convolution weights record it in their tail)
__global__ void cv_scale_kernel(const unsigned *__restrict__ bits, float *__restrict__ scale2) {
    store_scale2(scale2, __uint_as_float(*bits));
}

// ---- activation producers ------------------------------------------------------------------------------
// grid (ceil(HW/256), N*C/16): thread = pixel, 16 channel rows read coalesced, 4 plane pieces written.
// GN: z = act((x - mean)*rstd*gamma + beta) with per-group statistics; otherwise z = x * scale2[0].
template <bool GN, bool SILU>
__global__ void __launch_bounds__(256)
cv_to_split_kernel(const float *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                   const float *__restrict__ mean, const float *__restrict__ rstd, const float *__restrict__ scale2,
                   int C, int64_t HW, int cpg, uint4 *__restrict__ xs, int64_t sn, int64_t sc, int64_t sp, int prec,
                   const double *__restrict__ part = nullptr, int chunks = 0, float eps = 0.f,
                   float *__restrict__ mean_out = nullptr, float *__restrict__ rstd_out = nullptr) {
    __shared__ float pa[16], pb[16], pm[16];
    const int CK = C / 16;
    const int ck = (int)(blockIdx.y % CK);
    const int64_t n = blockIdx.y / CK;
    if (GN) {
        const int G = C / cpg;
        if (part) {
            // Statistics straight from the moment partials of gn_moments_kernel (csrc/group_norm.hip): each of the <= 5
            // groups this block's 16 channels touch is summed by one wave in gn_finalize_kernel's order (lane-strided,
            // then the xor tree), so mean / rstd are bit-identical to that kernel's -- whose launch this saves when
            // nobody else needs them (the no-grad forwards: the whole UNet and the masked-image encode).
            __shared__ float gmean[8], grstd[8];
            const int g0 = (ck * 16) / cpg, g1 = (ck * 16 + 15) / cpg;
            const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
            for (int gi = wave; gi <= g1 - g0; gi += 4) {
                const int64_t pbase = (n * C + (int64_t)(g0 + gi) * cpg) * chunks;
                const int P = cpg * chunks;
                double sm = 0.0, q = 0.0;
                for (int i = lane; i < P; i += 64) { sm += part[(pbase + i) * 2]; q += part[(pbase + i) * 2 + 1]; }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 64); q += __shfl_xor(q, o, 64); }
                if (lane == 0) {
                    const double m = (double)cpg * (double)HW;
                    const double mu = sm / m;
                    double var = q / m - mu * mu;
                    if (var < 0.0) var = 0.0;
                    gmean[gi] = (float)mu;
                    grstd[gi] = (float)(1.0 / sqrt(var + (double)eps));
                    // the statistics also leave for a backward that needs them (the first pixel block of every channel chunk
                    // writes its groups; chunks that share a group write the same bits): no gn_finalize launch
                    if (mean_out && blockIdx.x == 0) { mean_out[n * G + g0 + gi] = gmean[gi]; rstd_out[n * G + g0 + gi] = grstd[gi]; }
                }
            }
            __syncthreads();
            if (threadIdx.x < 16) {
                const int c = ck * 16 + threadIdx.x;
                const int gi = c / cpg - g0;
                pm[threadIdx.x] = gmean[gi];
                pa[threadIdx.x] = grstd[gi] * (gamma ? gamma[c] : 1.f);
                pb[threadIdx.x] = beta ? beta[c] : 0.f;
            }
        } else if (threadIdx.x < 16) {
            const int c = ck * 16 + threadIdx.x;
            const int g = c / cpg;
            pm[threadIdx.x] = mean[n * G + g];
            pa[threadIdx.x] = rstd[n * G + g] * (gamma ? gamma[c] : 1.f);
            pb[threadIdx.x] = beta ? beta[c] : 0.f;
        }
        __syncthreads();
    }
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float s = (!GN && scale2) ? scale2[0] : 1.f;
    const float *xr = x + n * sn + (int64_t)(ck * 16) * sc + p * sp;      // element (n, channel, pixel)
    float v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = xr[c * sc];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (GN) {
            const float z = (v[c] - pm[c]) * pa[c] + pb[c];
            // SiLU with v_rcp_f32 (1 ulp) instead of the ten-instruction IEEE divide: this writer is partly VALU-bound
            // (84 launches of the SDS step 1.13 -> 1.02 ms); the result is rounded to fp16 hi + lo (2^-22) right below
            v[c] = SILU ? z * __builtin_amdgcn_rcpf(1.0f + expf(-z)) : z;
        } else {
            v[c] *= s;
        }
    }
    uint4 *dst = xs + ((n * CK + ck) * 4) * HW + p;
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = v[kg * 8 + j];
        uint4 hi, lo;
        split8(t, hi, lo);
        dst[(kg * 2 + 0) * HW] = hi;
        if (prec != 1) dst[(kg * 2 + 1) * HW] = lo;          // prec 1 (fp16 mode): consumers fetch the hi plane only
    }
}

// Nearest-neighbour 2x up-sampling folded into the plane writer (Upsample2D of the UNet, F.interpolate(scale_factor=2) in
// front of a 3x3 convolution): output pixel (oy, ox) of the [2H, 2W] image reads x[oy / 2][ox / 2]; the up-sampled fp32
// tensor never exists.  grid (ceil(4HW/256), N*C/16).
__global__ void __launch_bounds__(256)
cv_to_split_up2_kernel(const float *__restrict__ x, const float *__restrict__ scale2, int C, int H, int W,
                       uint4 *__restrict__ xs, int prec) {
    const int CK = C / 16;
    const int ck = (int)(blockIdx.y % CK);
    const int64_t n = blockIdx.y / CK;
    const int64_t OHW = (int64_t)4 * H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= OHW) return;
    const int oy = (int)(p / (2 * W)), ox = (int)(p - (int64_t)oy * 2 * W);
    const float s = scale2 ? scale2[0] : 1.f;
    const float *xr = x + (n * C + (int64_t)ck * 16) * H * W + (int64_t)(oy >> 1) * W + (ox >> 1);
    float v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = xr[(int64_t)c * H * W] * s;
    uint4 *dst = xs + ((n * CK + ck) * 4) * OHW + p;
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = v[kg * 8 + j];
        uint4 hi, lo;
        split8(t, hi, lo);
        dst[(kg * 2 + 0) * OHW] = hi;
        if (prec != 1) dst[(kg * 2 + 1) * OHW] = lo;
    }
}

// ---- general convolution as a GEMM: the strided and the narrow-channel layers -----------------------------------
// (the three stride-2 down-samplers of the UNet and of the VAE encoder, conv_in / conv_out with 3, 4, 8 or 9 channels,
// quant_conv: DS_NeRF/guidance/sd_utils.py:207, :240 -- none fits the 3x3 stride-1 kernel's 16 / 32-channel operand tiles)
//   X_col[k = ci*KH*KW + ky*KW + kx][p = oy*OW + ox] = x[ci][oy*stride + ky - pad_top][ox*stride + kx - pad_left]
// written DIRECTLY as fp16 hi/lo split planes [N][KP/16][2][2][PP][8] (KP, PP: K and P padded to the GEMM's multiples, zero
// filled), so the convolution is mvip_gemm_f16x3 with the natural weight [Cout][Cin*KH*KW] as the A operand; the data
// gradient is the GEMM with A^T into col[N][KP][PP] followed by the gather below.
// grid (ceil(PP/256), N*KP/16): thread = output pixel, 16 consecutive k.
// KH_T, KW_T > 0: the kernel size as a compile-time constant (3 x 3 and 1 x 1: every layer of the SDS networks) -- the 32
// divisions by `taps` and KW per thread become multiplications; with run-time divisors this writer was bound by them.
template <int KH_T, int KW_T>
__global__ void __launch_bounds__(256)
cv_im2col_split_kernel(const float *__restrict__ x, int Cin, int H, int W, int KH_, int KW_, int stride, int pad_top,
                       int pad_left, int OH, int OW, int KP, int64_t PP, const float *__restrict__ scale2,
                       uint4 *__restrict__ xs, int prec) {
    const int KH = KH_T > 0 ? KH_T : KH_, KW = KW_T > 0 ? KW_T : KW_;
    const int CKP = KP / 16;
    const int ck = (int)(blockIdx.y % CKP);
    const int64_t n = blockIdx.y / CKP;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= PP) return;
    const float s = scale2 ? scale2[0] : 1.f;
    const int taps = KH * KW, K = Cin * taps;
    const bool inside = p < (int64_t)OH * OW;
    const unsigned pu = (unsigned)p;                                   // OH * OW <= 2^30 (checked by the caller)
    const int oy = inside ? (int)(pu / (unsigned)OW) : 0, ox = inside ? (int)(pu - (unsigned)oy * (unsigned)OW) : 0;
    const float *xn = x + n * Cin * H * W;
    // all 16 gathers are issued before any is used: a load under its own `if` is followed by s_waitcnt vmcnt(0), i.e. 16
    // exposed memory latencies per thread (invalid taps read element 0 and are zeroed afterwards)
    float v[16];
    int64_t src[16];
    bool ok[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int k = ck * 16 + c;
        const int kk = k < K ? k : 0;
        const int ci = kk / taps, t = kk - ci * taps;
        const int ky = t / KW, kx = t - ky * KW;
        const int iy = oy * stride + ky - pad_top, ix = ox * stride + kx - pad_left;
        ok[c] = inside && k < K && iy >= 0 && iy < H && ix >= 0 && ix < W;
        src[c] = ok[c] ? ((int64_t)ci * H + iy) * W + ix : 0;
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = xn[src[c]];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = ok[c] ? v[c] * s : 0.f;
    uint4 *dst = xs + ((n * CKP + ck) * 4) * PP + p;
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
        float t8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t8[j] = v[kg * 8 + j];
        uint4 hi, lo;
        split8(t8, hi, lo);
        dst[(kg * 2 + 0) * PP] = hi;
        if (prec != 1) dst[(kg * 2 + 1) * PP] = lo;
    }
}

// dx[n][ci][iy][ix] = sum over the (ky, kx) whose output pixel exists of col[n][ci*KH*KW + ky*KW + kx][oy*OW + ox]:
// a gather (deterministic), one thread per input element; grid (ceil(H W / 256), N * Cin).  KH_T, KW_T, ST_T > 0: kernel
// size and stride as compile-time constants (the tap loops unroll, `% stride` and `/ stride` become shifts, and the flat
// 64-bit index with its four divisions per thread is gone: that arithmetic, not memory, bounded the run-time version).
template <int KH_T, int KW_T, int ST_T>
__global__ void __launch_bounds__(256)
cv_col2im_kernel(const float *__restrict__ col, int Cin, int H, int W, int KH_, int KW_, int stride_, int pad_top, int pad_left,
                 int OH, int OW, int KP, int64_t PP, float *__restrict__ dx) {
    const int KH = KH_T > 0 ? KH_T : KH_, KW = KW_T > 0 ? KW_T : KW_, stride = ST_T > 0 ? ST_T : stride_;
    const unsigned p = blockIdx.x * 256u + threadIdx.x;                  // H * W <= 2^30 (checked by the caller)
    if (p >= (unsigned)(H * W)) return;
    const int iy = (int)(p / (unsigned)W), ix = (int)(p - (unsigned)iy * (unsigned)W);
    const int ci = (int)(blockIdx.y % (unsigned)Cin);
    const int64_t n = blockIdx.y / (unsigned)Cin;
    const float *cn = col + n * KP * PP;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < KH; ++ky) {
        const int ty = iy + pad_top - ky;
        if (ty < 0 || ty % stride != 0) continue;
        const int oy = ty / stride;
        if (oy >= OH) continue;
#pragma unroll
        for (int kx = 0; kx < KW; ++kx) {
            const int tx = ix + pad_left - kx;
            if (tx < 0 || tx % stride != 0) continue;
            const int ox = tx / stride;
            if (ox >= OW) continue;
            acc += cn[(int64_t)(ci * KH * KW + ky * KW + kx) * PP + (int64_t)oy * OW + ox];
        }
    }
    dx[((n * Cin + ci) * H + iy) * (int64_t)W + ix] = acc;
}

}  // namespace mvip

using namespace mvip;

void mvip::launch_absmax_then_scale(const float *x, int64_t n, unsigned *bits, float *scale2, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(cv_absmax_kernel, dim3(absmax_blocks(n)), dim3(256), 0, st, x, n, bits);
    hipLaunchKernelGGL(cv_scale_kernel, dim3(1), dim3(1), 0, st, (const unsigned *)bits, scale2);
}

void mvip::launch_absmax_scale(const float *x, int64_t n, unsigned *words2, float *scale2, hipStream_t st) {
    hipLaunchKernelGGL(cv_absmax_scale_kernel, dim3(absmax_blocks(n)), dim3(256), 0, st, x, n, words2, scale2);
}

// 1 in *two_product_host when every lo fragment of a packed weight image is zero, i.e. the scaled weights are exact fp16
// values and `prec = 2` (two products) gives the three-product result bit for bit.  `fragment_bytes` = the image's size
// without its 256-byte tail (Cout * Cin * 36 for mvip_conv3x3_pack, M * K * 4 for mvip_gemm_pack_a).  Reads ONE word back
// to the host after synchronising `stream`: a pack-time query, not for the step.
extern "C" int mvip_packed_weights_two_product(const void *packed, int64_t fragment_bytes, int *two_product_host, void *stream) {
    if (!packed || !two_product_host || fragment_bytes <= 0) return MVIP_EINVAL;
    unsigned flag = 1u;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemcpyAsync(&flag, (const char *)packed + fragment_bytes + 12, sizeof(flag), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { set_last_error(e); return MVIP_ELAUNCH; }
    *two_product_host = flag == 0u ? 1 : 0;
    return MVIP_OK;
}

extern "C" int mvip_absmax_scale(const float *x, int64_t n, float *scale2, void *zero_words2, void *stream) {
    if (n < 0 || !scale2 || (n > 0 && !x)) return MVIP_EINVAL;
    hipStream_t st = as_stream(stream);
    if (zero_words2 && n > 0) {                 // one launch: caller-owned scratch words that are zero between calls
        launch_absmax_scale(x, n, (unsigned *)zero_words2, scale2, st);
        return check_launch();
    }
    zero_words(scale2, 4, st);
    launch_absmax_then_scale(x, n, (unsigned *)(scale2 + 2), scale2, st);
    return check_launch();
}

extern "C" int mvip_split_planes(const float *x, int64_t N, int64_t C, int64_t HW, const float *scale2, void *xs, int prec,
                                 void *stream) {
    if (N < 0 || C <= 0 || C % 16 != 0 || HW < 0 || (prec < 0 || prec > 2)) return MVIP_EINVAL;
    if (N == 0 || HW == 0) return MVIP_OK;
    if (!x || !xs || N * (C / 16) > 65535) return MVIP_EINVAL;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(N * (C / 16)));
    hipLaunchKernelGGL((cv_to_split_kernel<false, false>), grid, dim3(256), 0, as_stream(stream), x, nullptr, nullptr,
                       nullptr, nullptr, scale2, (int)C, HW, 1, (uint4 *)xs, C * HW, HW, (int64_t)1, prec);
    return check_launch();
}

extern "C" int mvip_split_planes_upsample2(const float *x, int64_t N, int64_t C, int64_t H, int64_t W, const float *scale2,
                                           void *xs, int prec, void *stream) {
    if (N < 0 || C <= 0 || C % 16 != 0 || H <= 0 || W <= 0 || H * W > (1 << 26) || (prec < 0 || prec > 2)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!x || !xs || N * (C / 16) > 65535) return MVIP_EINVAL;
    const dim3 grid((unsigned)((4 * H * W + 255) / 256), (unsigned)(N * (C / 16)));
    hipLaunchKernelGGL(cv_to_split_up2_kernel, grid, dim3(256), 0, as_stream(stream), x, scale2, (int)C, (int)H, (int)W,
                       (uint4 *)xs, prec);
    return check_launch();
}

extern "C" int mvip_im2col_split_planes(const float *x, int64_t N, int64_t Cin, int64_t H, int64_t W, int KH, int KW,
                                        int stride, int pad_top, int pad_left, int64_t OH, int64_t OW, int64_t KP,
                                        int64_t PP, const float *scale2, void *xs, int prec, void *stream) {
    if ((prec < 0 || prec > 2) || N < 0 || Cin <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad_top < 0 || pad_left < 0 ||
        OH <= 0 || OW <= 0 || KP <= 0 || KP % 16 != 0 || KP < Cin * KH * KW || PP < OH * OW || H * W > (1 << 30) ||
        OH * OW > (1 << 30))
        return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!x || !xs || N * (KP / 16) > 65535) return MVIP_EINVAL;
    const dim3 grid((unsigned)((PP + 255) / 256), (unsigned)(N * (KP / 16)));
#define MVIP_I2C(A, B) hipLaunchKernelGGL((cv_im2col_split_kernel<A, B>), grid, dim3(256), 0, as_stream(stream), x, (int)Cin, (int)H, \
                                          (int)W, KH, KW, stride, pad_top, pad_left, (int)OH, (int)OW, (int)KP, PP, scale2,      \
                                          (uint4 *)xs, prec)
    if (KH == 3 && KW == 3) MVIP_I2C(3, 3); else if (KH == 1 && KW == 1) MVIP_I2C(1, 1); else MVIP_I2C(0, 0);
#undef MVIP_I2C
    return check_launch();
}

extern "C" int mvip_col2im(const float *col, int64_t N, int64_t Cin, int64_t H, int64_t W, int KH, int KW, int stride,
                           int pad_top, int pad_left, int64_t OH, int64_t OW, int64_t KP, int64_t PP, float *dx,
                           void *stream) {
    if (N < 0 || Cin <= 0 || H <= 0 || W <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad_top < 0 || pad_left < 0 ||
        OH <= 0 || OW <= 0 || KP < Cin * KH * KW || PP < OH * OW || H * W > (1 << 30) || OH * OW > (1 << 30))
        return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!col || !dx) return MVIP_EINVAL;
    if (N * Cin > 65535) return MVIP_EINVAL;
    const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)(N * Cin));
#define MVIP_C2I(A, B, C) hipLaunchKernelGGL((cv_col2im_kernel<A, B, C>), grid, dim3(256), 0, as_stream(stream), col, (int)Cin, (int)H, \
                                             (int)W, KH, KW, stride, pad_top, pad_left, (int)OH, (int)OW, (int)KP, PP, dx)
    if (KH == 3 && KW == 3 && stride == 2) MVIP_C2I(3, 3, 2);
    else if (KH == 3 && KW == 3 && stride == 1) MVIP_C2I(3, 3, 1);
    else if (KH == 1 && KW == 1 && stride == 1) MVIP_C2I(1, 1, 1);
    else MVIP_C2I(0, 0, 0);
#undef MVIP_C2I
    return check_launch();
}

extern "C" int mvip_split_planes_strided(const float *x, int64_t N, int64_t C, int64_t HW, int64_t sn, int64_t sc,
                                         int64_t sp, const float *scale2, void *xs, int prec, void *stream) {
    if (N < 0 || C <= 0 || C % 16 != 0 || HW < 0 || (prec < 0 || prec > 2)) return MVIP_EINVAL;
    if (N == 0 || HW == 0) return MVIP_OK;
    if (!x || !xs || N * (C / 16) > 65535) return MVIP_EINVAL;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(N * (C / 16)));
    hipLaunchKernelGGL((cv_to_split_kernel<false, false>), grid, dim3(256), 0, as_stream(stream), x, nullptr, nullptr,
                       nullptr, nullptr, scale2, (int)C, HW, 1, (uint4 *)xs, sn, sc, sp, prec);
    return check_launch();
}

extern "C" int mvip_groupnorm_split_planes(const float *x, const float *gamma, const float *beta, const float *mean,
                                           const float *rstd, int64_t N, int64_t C, int64_t HW, int G, int silu,
                                           void *xs, int prec, void *stream) {
    if (N < 0 || C <= 0 || C % 16 != 0 || HW < 0 || G <= 0 || C % G != 0 || (prec < 0 || prec > 2)) return MVIP_EINVAL;
    if (N == 0 || HW == 0) return MVIP_OK;
    if (!x || !xs || !mean || !rstd || N * (C / 16) > 65535) return MVIP_EINVAL;
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(N * (C / 16)));
    if (silu)
        hipLaunchKernelGGL((cv_to_split_kernel<true, true>), grid, dim3(256), 0, as_stream(stream), x, gamma, beta, mean,
                           rstd, nullptr, (int)C, HW, (int)(C / G), (uint4 *)xs, C * HW, HW, (int64_t)1, prec);
    else
        hipLaunchKernelGGL((cv_to_split_kernel<true, false>), grid, dim3(256), 0, as_stream(stream), x, gamma, beta, mean,
                           rstd, nullptr, (int)C, HW, (int)(C / G), (uint4 *)xs, C * HW, HW, (int64_t)1, prec);
    return check_launch();
}

extern "C" int mvip_groupnorm_split_planes_moments(const float *x, const float *gamma, const float *beta,
                                                   const void *moments, float eps, int64_t N, int64_t C, int64_t HW, int G,
                                                   int silu, void *xs, int prec, void *stream) {
    if (N < 0 || C <= 0 || C % 16 != 0 || HW < 0 || G <= 0 || C % G != 0 || (prec < 0 || prec > 2)) return MVIP_EINVAL;
    if (N == 0 || HW == 0) return MVIP_OK;
    if (!x || !xs || !moments || N * (C / 16) > 65535 || C / G < 4) return MVIP_EINVAL;          // <= 5 groups per 16 channels
    const int chunks = (int)(mvip_groupnorm_workspace_bytes(1, 1, HW) / 16);
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(N * (C / 16)));
    if (silu)
        hipLaunchKernelGGL((cv_to_split_kernel<true, true>), grid, dim3(256), 0, as_stream(stream), x, gamma, beta, nullptr,
                           nullptr, nullptr, (int)C, HW, (int)(C / G), (uint4 *)xs, C * HW, HW, (int64_t)1, prec,
                           (const double *)moments, chunks, eps);
    else
        hipLaunchKernelGGL((cv_to_split_kernel<true, false>), grid, dim3(256), 0, as_stream(stream), x, gamma, beta, nullptr,
                           nullptr, nullptr, (int)C, HW, (int)(C / G), (uint4 *)xs, C * HW, HW, (int64_t)1, prec,
                           (const double *)moments, chunks, eps);
    return check_launch();
}

// mvip_groupnorm_split_planes_moments that ALSO writes mean / rstd [N, G] (bit-identical to mvip_groupnorm_stats' own): the
// forward of a layer whose backward needs the statistics gets them from the plane writer, one launch less per GroupNorm.
extern "C" int mvip_groupnorm_split_planes_moments_out(const float *x, const float *gamma, const float *beta,
                                                       const void *moments, float eps, int64_t N, int64_t C, int64_t HW, int G,
                                                       int silu, void *xs, float *mean_out, float *rstd_out, int prec,
                                                       void *stream) {
    if (N < 0 || C <= 0 || C % 16 != 0 || HW < 0 || G <= 0 || C % G != 0 || (prec < 0 || prec > 2)) return MVIP_EINVAL;
    if (N == 0 || HW == 0) return MVIP_OK;
    if (!x || !xs || !moments || !mean_out || !rstd_out || N * (C / 16) > 65535 || C / G < 4) return MVIP_EINVAL;
    const int chunks = (int)(mvip_groupnorm_workspace_bytes(1, 1, HW) / 16);
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(N * (C / 16)));
    if (silu)
        hipLaunchKernelGGL((cv_to_split_kernel<true, true>), grid, dim3(256), 0, as_stream(stream), x, gamma, beta, nullptr,
                           nullptr, nullptr, (int)C, HW, (int)(C / G), (uint4 *)xs, C * HW, HW, (int64_t)1, prec,
                           (const double *)moments, chunks, eps, mean_out, rstd_out);
    else
        hipLaunchKernelGGL((cv_to_split_kernel<true, false>), grid, dim3(256), 0, as_stream(stream), x, gamma, beta, nullptr,
                           nullptr, nullptr, (int)C, HW, (int)(C / G), (uint4 *)xs, C * HW, HW, (int64_t)1, prec,
                           (const double *)moments, chunks, eps, mean_out, rstd_out);
    return check_launch();
}
