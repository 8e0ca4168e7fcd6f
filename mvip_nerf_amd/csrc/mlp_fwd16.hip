// Entry points of the two-waves-per-SIMD exact-fp32 forward (kernel: mlp_fwd16_kernel.h): the image pack, the unfolded
// inference launches and the stash-writing training forward.  The folded inference launches are mlp_fwd16_fold.hip.
#include "mlp_fwd16_kernel.h"
#include "mlp_image.h"

namespace mvip {
namespace f16p {

__global__ void mlp_pack16_kernel(ParamPtrs pp, float *__restrict__ packed) { pack_image<Frag16>(pp, packed); }

}  // namespace f16p
}  // namespace mvip

using namespace mvip;
using namespace mvip::f16p;

// packed16 = [section A in 16-point block order | section B copied from the 32-point image]
extern "C" int mvip_mlp_pack16(const float *const *params_host, const float *packed32, float *packed16, void *stream) {
    mlp::ParamPtrs pp;
    if (!mlp::collect_params(params_host, pp) || !packed32 || !packed16) return MVIP_EINVAL;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mlp_pack16_kernel, dim3(mlp::pack_image_grid<mlp::Frag16>()), dim3(mlp::PACK_THREADS), 0, st, pp, packed16);
    return mlp::finish_with_section_b(packed16, packed32, st);
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
