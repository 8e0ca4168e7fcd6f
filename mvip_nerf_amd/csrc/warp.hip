// Reference-view propagation: backward depth warping of source views into target views (beyond the reference, which has no
// counterpart: it reads RGB_inpainted/ as independent 2D inpaintings of every view; ops.warp_views, prepare.propagate_reference).
//
// Definition (the camera, its unproject / project / in_image / lower_footprint / lower_blend, is csrc/camera_device.h's; restated
// in tests/warp_numpy.py).  Per target n and pixel (y, x) whose mask byte is set and whose disparity is finite and > 0:
//   p_w = unproject(pose_n, x, y, t = 1 / disp)
//   for k = 0 .. S-1, s = order[n][k] (skipped unless 0 <= s < S), until a source is taken:
//     (u, v, t_s) = project(pose_s, p_w);  skipped unless in_image(t_s, u, v)
//     a = lower_blend of the lower_footprint of (u, v), for the source's disparity d_s and colour
//     resid = t_s d_s - 1;  taken iff in range, d_s finite and > 0, |resid| <= tol and the three colours finite.
// rgb / index / resid = the taken source's colour / s / resid, else 0 / -1 / 0 (also for unmasked and invalid pixels).
//
// Shape: a pure gather.  One thread per target pixel, lane = column, a workgroup is 64 columns x 4 rows; every pixel of every
// target is written, so the outputs need no clearing.  tgt_disp / tgt_mask are read coalesced; the poses and the order row are
// read at wave-uniform addresses (once per wave, into scalar registers); the four taps of the source's disparity are gathered
// first and the twelve colour taps only by the lanes whose residual passes.  Neighbouring lanes gather neighbouring source
// pixels, so the taps are served by L2.  No LDS, no atomics, no scratch; the only loop runs over the S entries of the order
// row.  Every index is bounded before it is used: x < W, y < H; taps only on lanes that are in range, where
// 0 <= x0 <= W-2 and 0 <= y0 <= H-2 by construction; 0 <= s < S.  Offsets are 64-bit.  A pixel's result depends on its own inputs
// only: target n of a batch equals the single-target call bit for bit, and a call equals its repetition.
//
// Bytes from HBM: per target pixel 5 read (disparity, mask) + 20 written; each source's 16 B per pixel (disparity, colour) at most
// once, the gathers' repeats being served by L2 and the Infinity Cache (tools/warp_bench.py::hbm_bytes).
#include "camera_device.h"

namespace mvip {
namespace warp {

namespace cam = mvip::camera;

__global__ __launch_bounds__(cam::TILE) void warp_kernel(const float *__restrict__ tgt_disp, const float *__restrict__ tgt_pose,
                                                        const unsigned char *__restrict__ tgt_mask, const cam::PixelTiles s,
                                                        const float *__restrict__ src_rgb, const float *__restrict__ src_disp,
                                                        const float *__restrict__ src_pose, const int S, const int *__restrict__ order,
                                                        const float focal, const float tol, float *__restrict__ rgb,
                                                        int *__restrict__ index, float *__restrict__ resid) {
    int n, x, y;
    if (!cam::tile_pixel(s, n, x, y)) return;
    const long long p = n * s.HW + (long long)y * s.W + x;
    const float d = tgt_disp[p];
    float out_r = 0.f, out_g = 0.f, out_b = 0.f, out_e = 0.f;
    int out_i = -1;
    const bool seen = cam::usable(d);
    if (tgt_mask[p] != 0 && seen) {
        float pw0, pw1, pw2;
        cam::unproject<float>(tgt_pose + (long long)n * 12, s.H, s.W, focal, x, y, 1.0f / d, pw0, pw1, pw2);
        const float cu = (float)s.W * .5f, cv = (float)s.H * .5f;
        for (int k = 0; k < S && out_i < 0; ++k) {
            const int src = order[(long long)n * S + k];
            if (src < 0 || src >= S) continue;
            float u, v, ts;
            cam::project<float>(src_pose + (long long)src * 12, focal, cu, cv, pw0, pw1, pw2, u, v, ts);
            if (!cam::in_image(ts, u, v, s.H, s.W)) continue;
            int x0, y0;
            float fx, fy;
            cam::lower_footprint(u, v, s.H, s.W, x0, y0, fx, fy);
            const long long a = src * s.HW + (long long)y0 * s.W + x0, b = a + s.W;
            const float ds = cam::lower_blend(src_disp[a], src_disp[a + 1], src_disp[b], src_disp[b + 1], fx, fy);
            const float e = ts * ds - 1.0f;
            if (!(cam::usable(ds) && fabsf(e) <= tol)) continue;
            const float *__restrict__ ca = src_rgb + a * 3, *__restrict__ cb = src_rgb + b * 3;
            const float r = cam::lower_blend(ca[0], ca[3], cb[0], cb[3], fx, fy);
            const float g = cam::lower_blend(ca[1], ca[4], cb[1], cb[4], fx, fy);
            const float bl = cam::lower_blend(ca[2], ca[5], cb[2], cb[5], fx, fy);
            if (!(finite(r) && finite(g) && finite(bl))) continue;
            out_r = r; out_g = g; out_b = bl; out_e = e; out_i = src;
        }
    }
    rgb[p * 3 + 0] = out_r;
    rgb[p * 3 + 1] = out_g;
    rgb[p * 3 + 2] = out_b;
    index[p] = out_i;
    resid[p] = out_e;
}

}  // namespace warp
}  // namespace mvip

using namespace mvip;

extern "C" int mvip_warp_views(const float *tgt_disp, const float *tgt_pose, const void *tgt_mask, int64_t N, int H, int W,
                               const float *src_rgb, const float *src_disp, const float *src_pose, int S, const int *order,
                               float focal, float tol, float *rgb, int *index, float *resid, void *stream) {
    if (N < 0 || S < 0 || H < 2 || W < 2 || H > camera::MAX_SIDE || W > camera::MAX_SIDE) return MVIP_EINVAL;
    if (!camera::usable(focal) || !camera::usable(tol)) return MVIP_EINVAL;
    const camera::PixelTiles s = camera::make_tiles(H, W);
    if (N > (int64_t)INT32_MAX / s.T || (int64_t)S > (int64_t)INT32_MAX / 12) return MVIP_EINVAL;      // the grid, and n, fit an int
    if (N == 0) return MVIP_OK;
    if (!tgt_disp || !tgt_pose || !tgt_mask || !rgb || !index || !resid) return MVIP_EINVAL;
    if (S > 0 && (!src_rgb || !src_disp || !src_pose || !order)) return MVIP_EINVAL;
    hipLaunchKernelGGL(warp::warp_kernel, dim3((unsigned)(N * s.T)), dim3(camera::TILE), 0, as_stream(stream), tgt_disp, tgt_pose,
                       (const unsigned char *)tgt_mask, s, src_rgb, src_disp, src_pose, S, order, focal, tol, rgb, index, resid);
    return check_launch();
}
