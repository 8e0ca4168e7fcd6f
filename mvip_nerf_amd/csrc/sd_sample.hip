// The 2D inpainting sampler of the SDS prior (StableDiffusion.produce_latents / decode_latents / prompt_to_img / inpaint,
// DS_NeRF/guidance/sd_utils.py:602-666): the VAE decoder's tail and one DDIM update, one launch each.
#include "common.h"
#include <hip/hip_fp16.h>

namespace mvip {

// ---- decoder head: img = clamp(conv3x3(silu(group_norm(x)), W, b) / 2 + 0.5, 0, 1)   (conv_norm_out -> SiLU -> conv_out
// of AutoencoderKL's decoder, then decode_latents' post-processing, DS_NeRF/guidance/sd_utils.py:624-631)
// One workgroup = a 16 x 32 output tile of one image; the activated input tile (18 x 34 with its halo) is staged in LDS eight
// channels at a time, so every input value is read from memory and activated once per tile (the halo: 1.2x).  The zero padding
// of the convolution applies to the ACTIVATED input: out-of-image taps are 0, not silu(beta - gamma mean rstd).
// The next stage's loads are issued before the current stage's products (register prefetch).  Each thread owns two vertically
// adjacent pixels: 12 LDS reads for 2 x 27 products per channel.
constexpr int DH_TW = 32, DH_TH = 16, DH_CC = 8, DH_THREADS = 256;
constexpr int DH_LW = DH_TW + 2, DH_LH = DH_TH + 2, DH_PLANE = DH_LW * DH_LH;
constexpr int DH_STAGE = DH_CC * DH_PLANE;
constexpr int DH_PER_THREAD = (DH_STAGE + DH_THREADS - 1) / DH_THREADS;

__device__ __forceinline__ float dh_round(float v, bool f16) { return f16 ? __half2float(__float2half(v)) : v; }
__device__ __forceinline__ float dh_load(const float *p, int64_t i) { return p[i]; }
__device__ __forceinline__ float dh_load(const __half *p, int64_t i) { return __half2float(p[i]); }

// F16: prec == 1 (the reference's --fp16 mode): activations and weights rounded to fp16, products exact in fp32, fp32 sums
template <typename T, bool F16>
__global__ void __launch_bounds__(DH_THREADS) vae_decoder_head_kernel(
        const T *__restrict__ x, const float *__restrict__ mean, const float *__restrict__ rstd,
        const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ wt,
        const float *__restrict__ bias, int C, int H, int W, int G, float *__restrict__ img, uint8_t *__restrict__ img_u8) {
    __shared__ float tile[DH_STAGE];
    __shared__ float st[2][2][DH_CC];                    // [buffer][scale | shift][channel of the stage]
    __shared__ __attribute__((aligned(16))) float wsh[2][DH_CC * 28];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * DH_TW, y0 = blockIdx.y * DH_TH;
    const int64_t HW = (int64_t)H * W;
    const T *xn = x + (int64_t)n * C * HW;
    const int cpg = C / G;

    // stage-independent part of every element's address (-1: outside the image or past the stage)
    int off[DH_PER_THREAD];
#pragma unroll
    for (int k = 0; k < DH_PER_THREAD; ++k) {
        const int e = tid + k * DH_THREADS;
        const int c = e / DH_PLANE, rem = e - c * DH_PLANE, r = rem / DH_LW, col = rem - r * DH_LW;
        const int gy = y0 - 1 + r, gx = x0 - 1 + col;
        off[k] = (e < DH_STAGE && gy >= 0 && gy < H && gx >= 0 && gx < W) ? c * (int)HW + gy * W + gx : -1;
    }
    // per stage: the 8 channels' GroupNorm scale / shift and their 3 x 9 weights ([channel][o * 9 + tap], padded to 28 for
    // float4 reads), double-buffered: written during the previous stage's products
    auto stage_params = [&](int c0, int buf) {
        if (tid < DH_CC) {
            const int c = c0 + tid, g = n * G + c / cpg;
            const float s = __fmul_rn(rstd[g], gamma[c]);
            st[buf][0][tid] = s;
            st[buf][1][tid] = __fsub_rn(beta[c], __fmul_rn(mean[g], s));
        }
        if (tid < DH_CC * 28) {
            const int cc = tid / 28, j = tid - cc * 28, o = j / 9, tap = j - o * 9;
            wsh[buf][tid] = j < 27 ? dh_round(wt[((int64_t)o * C + c0 + cc) * 9 + tap], F16) : 0.f;
        }
    };
    float v[DH_PER_THREAD];
    auto fetch = [&](int c0) {
        const T *xc = xn + (int64_t)c0 * HW;
#pragma unroll
        for (int k = 0; k < DH_PER_THREAD; ++k) v[k] = off[k] >= 0 ? dh_load(xc, off[k]) : 0.f;
    };

    const int tx = tid & (DH_TW - 1), ty = (tid / DH_TW) * 2;
    float acc0[3] = {0.f, 0.f, 0.f}, acc1[3] = {0.f, 0.f, 0.f};
    fetch(0);
    stage_params(0, 0);
    for (int c0 = 0, it = 0; c0 < C; c0 += DH_CC, ++it) {
        __syncthreads();                                 // the previous stage's products are done with `tile`; st visible
        const int buf = it & 1;
#pragma unroll
        for (int k = 0; k < DH_PER_THREAD; ++k) {
            const int e = tid + k * DH_THREADS;
            if (e < DH_STAGE) {
                float a = 0.f;
                if (off[k] >= 0) {
                    const int c = e / DH_PLANE;
                    const float h = __fadd_rn(__fmul_rn(v[k], st[buf][0][c]), st[buf][1][c]);
                    a = dh_round(h / (1.0f + expf(-h)), F16);            // SiLU as csrc/group_norm.hip's silu_f
                }
                tile[e] = a;
            }
        }
        __syncthreads();
        if (c0 + DH_CC < C) {                            // next stage in flight during this stage's products
            fetch(c0 + DH_CC);
            stage_params(c0 + DH_CC, buf ^ 1);
        }
#pragma unroll 2
        for (int cc = 0; cc < DH_CC; ++cc) {
            float t[4][3];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) t[r][q] = tile[cc * DH_PLANE + (ty + r) * DH_LW + tx + q];
            float w[28];
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const float4 w4 = *reinterpret_cast<const float4 *>(&wsh[buf][cc * 28 + 4 * q]);
                w[4 * q] = w4.x; w[4 * q + 1] = w4.y; w[4 * q + 2] = w4.z; w[4 * q + 3] = w4.w;
            }
#pragma unroll
            for (int o = 0; o < 3; ++o)
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float wv = w[o * 9 + dy * 3 + dx];
                        acc0[o] = __fmaf_rn(wv, t[dy][dx], acc0[o]);
                        acc1[o] = __fmaf_rn(wv, t[dy + 1][dx], acc1[o]);
                    }
        }
    }
    const int gx = x0 + tx;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int gy = y0 + ty + p;
        if (gy >= H || gx >= W) continue;
        const int64_t pix = (int64_t)gy * W + gx;
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const float y = __fadd_rn(p ? acc1[o] : acc0[o], bias[o]);
            const float im = fminf(fmaxf(__fadd_rn(__fmul_rn(y, 0.5f), 0.5f), 0.f), 1.f);
            img[((int64_t)n * 3 + o) * HW + pix] = im;
            if (img_u8) img_u8[((int64_t)n * HW + pix) * 3 + o] = (uint8_t)rintf(__fmul_rn(im, 255.f));   // round half to even
        }
    }
}

// ---- one DDIM update (eta = 0) with classifier-free guidance, scal = {g, sqrt(abar_t), sqrt(1 - abar_t), sqrt(abar_prev),
// sqrt(1 - abar_prev), t_next}:  eps = e_u + g (e_c - e_u);  x0 = (x - sqrt(1-abar_t) eps) / sqrt(abar_t);
// x <- sqrt(abar_prev) x0 + sqrt(1-abar_prev) eps.  The new latents also go to channels 0..3 of every batch entry of the next
// UNet input [B][in_ch][hw] (unet_in nullable) and t_next to the UNet's timestep word (t_out nullable).
__global__ void ddim_cfg_step_kernel(const float *__restrict__ eps, int cfg, const float *__restrict__ scal, float *__restrict__ x,
                                     int64_t hw, float *__restrict__ unet_in, int64_t in_ch, int batch, float *__restrict__ t_out) {
    const int64_t n = 4 * hw;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && t_out) t_out[0] = scal[5];
    if (i >= n) return;
    const float u = eps[i];
    const float e = cfg ? __fadd_rn(u, __fmul_rn(scal[0], __fsub_rn(eps[n + i], u))) : u;
    const float x0 = __fdiv_rn(__fsub_rn(x[i], __fmul_rn(scal[2], e)), scal[1]);
    const float xp = __fadd_rn(__fmul_rn(scal[3], x0), __fmul_rn(scal[4], e));
    x[i] = xp;
    if (unet_in) {
        const int64_t c = i / hw, p = i - c * hw;
        for (int b = 0; b < batch; ++b) unet_in[((int64_t)b * in_ch + c) * hw + p] = xp;
    }
}

}  // namespace mvip

using namespace mvip;

extern "C" int mvip_vae_decoder_head(const void *x, const float *mean, const float *rstd, const float *gamma, const float *beta,
                                     const float *weight, const float *bias, int64_t N, int64_t C, int64_t H, int64_t W, int G,
                                     int dtype, float *img, uint8_t *img_u8, int prec, void *stream) {
    if (N < 0 || C <= 0 || C % 32 != 0 || H <= 0 || W <= 0 || G <= 0 || C % G != 0 || N > 65535 || H > (1 << 20) ||
        W > (1 << 20) || H * W > (1LL << 27) || (dtype != 0 && dtype != 1) || prec < 0 || prec > 2)
        return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!x || !mean || !rstd || !gamma || !beta || !weight || !bias || !img) return MVIP_EINVAL;
    const dim3 grid((unsigned)((W + DH_TW - 1) / DH_TW), (unsigned)((H + DH_TH - 1) / DH_TH), (unsigned)N);
    const hipStream_t st = as_stream(stream);
#define MVIP_DH_LAUNCH(T, F16)                                                                                                  \
    hipLaunchKernelGGL((vae_decoder_head_kernel<T, F16>), grid, dim3(DH_THREADS), 0, st, (const T *)x, mean, rstd, gamma, beta, \
                       weight, bias, (int)C, (int)H, (int)W, G, img, img_u8)
    if (dtype == 0) {
        if (prec == 1) MVIP_DH_LAUNCH(float, true); else MVIP_DH_LAUNCH(float, false);
    } else {
        if (prec == 1) MVIP_DH_LAUNCH(__half, true); else MVIP_DH_LAUNCH(__half, false);
    }
#undef MVIP_DH_LAUNCH
    return check_launch();
}

extern "C" int mvip_ddim_cfg_step(const float *eps, int cfg, const float *scal, float *x, int64_t hw, float *unet_in,
                                  int64_t in_ch, float *t_out, void *stream) {
    if (hw <= 0 || hw > (1LL << 28) || (cfg != 0 && cfg != 1) || (unet_in && in_ch < 4)) return MVIP_EINVAL;
    if (!eps || !scal || !x) return MVIP_EINVAL;
    const int64_t n = 4 * hw;
    hipLaunchKernelGGL(ddim_cfg_step_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), eps, cfg, scal, x,
                       hw, unet_in, in_ch, cfg ? 2 : 1, t_out);
    return check_launch();
}
