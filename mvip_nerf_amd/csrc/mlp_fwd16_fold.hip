// The folded inference network on the two-waves-per-SIMD exact-fp32 kernel (mlp_fwd16_kernel.h, FOLD = true): the pack of the
// folded tail of the extended image and the folded twins of the four inference launches of mlp_fwd16.hip.
#include "mlp_fwd16_kernel.h"
#include "mlp_image.h"

namespace mvip {
namespace f16p {

// Tail of the extended image (mlp_layout.h): the folded view blocks W'' = [Wv[:, :256] Wf | Wv[:, 256:283] | 0] (128 x 288) in
// the view layer's block order, then a copy of section B with b' = Wv[:, :256] bf + bv at SB_BFOLD.
// Every sum runs over k = 0..255 in ascending order in fp64 (each product of two fp32 values is exact in fp64, so contraction
// cannot change it) and is rounded to fp32 once: the image is a deterministic function of the parameters, identical on every
// rank, and tests/test_fold_cpu.py restates it bit for bit in numpy.
// One workgroup per block (to, ti) = a 16 x 16 tile of W'', one thread per float; the 16 rows of Wv and the 16 columns of Wf
// the tile needs are staged in LDS first (one coalesced pass), so the 256-step sums read LDS instead of chasing global-memory
// latency 256 times.  The ti == 0 workgroups also form b' of their 16 rows; the last workgroup copies section B.
constexpr int FOLD_PACK_WV_LD = 257;                  // row pitch of the Wv tile in LDS (odd: the 16 rows hit 16 banks)
__global__ void __launch_bounds__(256) mlp_fold_pack16_kernel(ParamPtrs pp, float *__restrict__ packed) {
    __shared__ float swv[16 * FOLD_PACK_WV_LD];
    __shared__ float swf[256 * 16];
    __shared__ float sbf[256];
    const int t = threadIdx.x, blk = blockIdx.x;
    if (blk == FOLD_BLOCKS) {                          // section B: the plain image's (already packed on this stream), minus b'
        for (int j = t; j < SEC_B_FLOATS; j += 256)
            if (j < SB_BFOLD || j >= SB_BFOLD + 128) packed[FOLD_TAIL_B + j] = packed[SEC_A_FLOATS + j];
        return;
    }
    constexpr LayerRow LV = LAYER[L_VIEWS];            // the folded blocks have the view layer's shape, order and padding
    const float *wv = pp.p[P_WV], *wf = pp.p[P_WF];
    int row, col, lo;
    Frag16::decode(blk, t, LV.k_padded, row, col, lo);
    const int to = row >> 4, m = row & 15, ti = col >> 4, c = col & 15;
    float v;
    if (ti < 16) {
#pragma unroll
        for (int r = 0; r < 16; ++r) swv[r * FOLD_PACK_WV_LD + t] = wv[(16 * to + r) * LV.k_real + t];
#pragma unroll
        for (int j = 0; j < 16; ++j) swf[(16 * j + t / 16) * 16 + t % 16] = wf[(16 * j + t / 16) * 256 + 16 * ti + t % 16];
        if (ti == 0) sbf[t] = pp.p[P_BF][t];
        __syncthreads();
        double acc = 0.0;
#pragma unroll 16
        for (int k = 0; k < 256; ++k) acc += (double)swv[m * FOLD_PACK_WV_LD + k] * (double)swf[k * 16 + c];
        v = (float)acc;
        if (ti == 0 && t < 16) {
            double b = 0.0;
#pragma unroll 16
            for (int k = 0; k < 256; ++k) b += (double)swv[t * FOLD_PACK_WV_LD + k] * (double)sbf[k];
            packed[FOLD_TAIL_B + SB_BFOLD + 16 * to + t] = (float)(b + (double)pp.p[P_BV][16 * to + t]);
        }
    } else {
        v = weight_at(pp, LV, row, col);
    }
    packed[FOLD_TAIL_A + blk * BLOCK_FLOATS + t] = v;
}

}  // namespace f16p
}  // namespace mvip

using namespace mvip;
using namespace mvip::f16p;

extern "C" int64_t mvip_mlp_packed_fold_floats(void) { return mlp::PACKED_FOLD_FLOATS; }

// Fills the tail of an extended image (mvip_mlp_packed_fold_floats() floats) whose first mvip_mlp_packed_floats() floats
// mvip_mlp_pack16 has already written on this stream: the folded view blocks and the section-B copy with the folded bias.
extern "C" int mvip_mlp_fold_pack16(const float *const *params_host, float *packed16_ext, void *stream) {
    mlp::ParamPtrs pp;
    if (!mlp::collect_params(params_host, pp) || !packed16_ext) return MVIP_EINVAL;
    hipLaunchKernelGGL(mlp_fold_pack16_kernel, dim3(mlp::FOLD_BLOCKS + 1), dim3(256), 0, as_stream(stream), pp, packed16_ext);
    return check_launch();
}

extern "C" int mvip_mlp_forward_rays16_fold(const float *packed16_ext, const float *rows, const float *z, int64_t B, int S,
                                            float *raw, void *stream) {
    return forward_rays16<true>(packed16_ext, rows, z, B, S, raw, stream);
}

extern "C" int mvip_mlp_forward_points16_fold(const float *packed16_ext, const float *pts, const float *dirs, int64_t P,
                                              float *raw, void *stream) {
    return forward_points16<true>(packed16_ext, pts, dirs, P, raw, stream);
}

extern "C" int mvip_render_coarse_fused_fold(const float *packed16_ext, const float *rows, int64_t B, const float *t_vals,
                                             int lindisp, const float *t_rand, const float *noise, const float *u, int u_is_row,
                                             int Nf, int flags, float *rgb0, float *disp0, float *acc0, float *depth0,
                                             float *weights0, float *alpha0, float *z_merged, float *z_std, void *stream) {
    return render_coarse_fused<true>(packed16_ext, rows, B, t_vals, lindisp, t_rand, noise, u, u_is_row, Nf, flags, rgb0, disp0,
                                     acc0, depth0, weights0, alpha0, z_merged, z_std, stream);
}

extern "C" int mvip_render_fine_fused_fold(const float *packed16_ext, const float *rows, const float *z, int64_t B,
                                           const float *noise, int flags, float *raw, float *rgb, float *disp, float *acc,
                                           float *depth, float *weights, float *alpha, void *stream) {
    return render_fine_fused<true>(packed16_ext, rows, z, B, noise, flags, raw, rgb, disp, acc, depth, weights, alpha, stream);
}
