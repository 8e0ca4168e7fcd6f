// Entry points of the two-waves-per-SIMD exact-fp32 forward (kernel: mlp_fwd16_kernel.h): the image pack, the unfolded
// inference launches and the stash-writing training forward.  The folded inference launches are mlp_fwd16_fold.hip.
#include "mlp_fwd16_kernel.h"

namespace mvip {
namespace f16p {

// ---- packing ---------------------------------------------------------------------------------------------------
__global__ void mlp_pack16_kernel(ParamPtrsC16 pp, float *__restrict__ packed) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= SEC_A_FLOATS) return;
    const int blk = idx / BLOCK_FLOATS, r = idx % BLOCK_FLOATS;
    const int lane = r / 4, s = r % 4, m = lane & 15, g = lane >> 4;
    int local, nti, param;
    int layer = -1;                                   // 0..7 hidden, 8 feature, 9 views
    if (blk < OFF_L1) { local = blk; nti = NTI_L0; layer = 0; }
    else if (blk < OFF_L5) { layer = 1 + (blk - OFF_L1) / LH_BLOCKS; local = (blk - OFF_L1) % LH_BLOCKS; nti = NTI_LH; }
    else if (blk < OFF_L6) { layer = 5; local = blk - OFF_L5; nti = NTI_L5; }
    else if (blk < OFF_FEAT) { layer = 6 + (blk - OFF_L6) / LH_BLOCKS; local = (blk - OFF_L6) % LH_BLOCKS; nti = NTI_LH; }
    else if (blk < OFF_VIEWS) { layer = 8; local = blk - OFF_FEAT; nti = NTI_LH; }
    else { layer = 9; local = blk - OFF_VIEWS; nti = NTI_LV; }
    const int to = local / nti, ti = local % nti;
    const int row = 16 * to + m, col = 16 * ti + 4 * g + s;
    float v = 0.f;
    if (layer == 0) { if (col < 63) v = pp.p[P_W0][row * 63 + col]; }
    else if (layer == 5) {
        if (col < 63) v = pp.p[10][row * 319 + col];
        else if (col >= 64) v = pp.p[10][row * 319 + 63 + (col - 64)];
    }
    else if (layer == 8) v = pp.p[P_WF][row * 256 + col];
    else if (layer == 9) { if (col < 283) v = pp.p[P_WV][row * 283 + col]; }
    else { param = 2 * layer; v = pp.p[param][row * 256 + col]; }
    packed[idx] = v;
}

}  // namespace f16p
}  // namespace mvip

using namespace mvip;
using namespace mvip::f16p;

// packed16 = [section A in 16-point block order | section B copied from the 32-point image]
extern "C" int mvip_mlp_pack16(const float *const *params_host, const float *packed32, float *packed16, void *stream) {
    if (!params_host || !packed32 || !packed16) return MVIP_EINVAL;
    ParamPtrsC16 pp;
    for (int i = 0; i < mlp::P_COUNT; ++i) {
        if (!params_host[i]) return MVIP_EINVAL;
        pp.p[i] = params_host[i];
    }
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mlp_pack16_kernel, dim3((mlp::SEC_A_FLOATS + 255) / 256), dim3(256), 0, st, pp, packed16);
    if (hipMemcpyAsync(packed16 + mlp::SEC_A_FLOATS, packed32 + mlp::SEC_A_FLOATS, mlp::SEC_B_FLOATS * sizeof(float),
                       hipMemcpyDeviceToDevice, st) != hipSuccess)
        return check_launch();
    return check_launch();
}

extern "C" int mvip_mlp_forward_rays16(const float *packed16, const float *rows, const float *z, int64_t B, int S,
                                       float *raw, void *stream) {
    return forward_rays16<false>(packed16, rows, z, B, S, raw, stream);
}

// Training forward on the two-wave kernel: raw AND the activation stash of mvip_mlp_stash_floats(B*S) floats that
// mvip_mlp_backward_stash consumes (same layout as mvip_mlp_forward_rays_stash writes; precision 0 only).
extern "C" int mvip_mlp_forward_rays_stash16(const float *packed16, const float *rows, const float *z, int64_t B, int S,
                                             float *raw, float *stash, void *stream) {
    if (B < 0 || S <= 0) return MVIP_EINVAL;
    if (B == 0) return MVIP_OK;
    if (!packed16 || !rows || !z || !raw || !stash) return MVIP_EINVAL;
    const int64_t P = B * S;
    const int64_t wgs = (P + WG_POINTS - 1) / WG_POINTS;
    hipLaunchKernelGGL((mlp_forward16_kernel<true, true>), dim3((unsigned)wgs), dim3(512), 0, as_stream(stream), packed16,
                       rows, z, P, S, raw, stash, wgs * 4);
    return check_launch();
}

extern "C" int mvip_mlp_forward_points16(const float *packed16, const float *pts, const float *dirs, int64_t P,
                                         float *raw, void *stream) {
    return forward_points16<false>(packed16, pts, dirs, P, raw, stream);
}

extern "C" int mvip_render_coarse_fused(const float *packed16, const float *rows, int64_t B, const float *t_vals, int lindisp,
                                        const float *t_rand, const float *noise, const float *u, int u_is_row, int Nf, int flags,
                                        float *rgb0, float *disp0, float *acc0, float *depth0, float *weights0, float *alpha0,
                                        float *z_merged, float *z_std, void *stream) {
    return render_coarse_fused<false>(packed16, rows, B, t_vals, lindisp, t_rand, noise, u, u_is_row, Nf, flags, rgb0, disp0, acc0,
                                      depth0, weights0, alpha0, z_merged, z_std, stream);
}

extern "C" int mvip_render_fine_fused(const float *packed16, const float *rows, const float *z, int64_t B, const float *noise,
                                      int flags, float *raw, float *rgb, float *disp, float *acc, float *depth, float *weights,
                                      float *alpha, void *stream) {
    return render_fine_fused<false>(packed16, rows, z, B, noise, flags, raw, rgb, disp, acc, depth, weights, alpha, stream);
}
