// Cross-view depth consistency: per pixel of every view, how many other views see a surface at the same place (agreement) and
// how many see THROUGH that place to something farther (a free-space violation, the signature of a floater).  Beyond the
// reference, which has no counterpart (ops.depth_consistency, prepare.consistency_mask).
//
// Definition, in fp64 on the fp32 inputs (the camera, its unproject / project / in_image / lower_footprint / lower_blend, is
// csrc/camera_device.h's, here with T = double; restated in tests/depth_consistency_numpy.py).  A target is a pixel (y, x) of
// view n whose disparity d is finite and > 0:
//   p_w = unproject(pose_n, x, y, t = 1 / d)
//   for every view s != n, in ascending s:
//     (u, v, t_s) = project(pose_s, p_w);  in range: in_image(t_s, u, v)
//     valid: ALL FOUR taps of view s's disparity at the lower_footprint of (u, v) finite and > 0 (the four-pixel rule of
//            csrc/texture.hip: a caller masks a pixel by zeroing it)
//     d_s = lower_blend of the four taps;  resid = t_s d_s - 1
//     in range and valid and |resid| <= tol:  agree[n,y,x] += 1
//     in range and valid and resid < -tol:    violated[n,y,x] += 1   (view s sees a farther surface along a ray through the point)
//     resid > tol: the point is occluded in s -- no evidence, nothing counted
// A pixel that is not a target gets 0 / 0.  Every element of both outputs is written.
//
// Shape: a pure gather, as csrc/warp.hip.  One thread per target pixel, lane = column, a workgroup is 64 columns x 4 rows; the
// view loop runs over s = 0 .. V-1 for the whole wave, the poses are read at wave-uniform addresses.  Neighbouring lanes
// gather neighbouring source pixels, so the taps are served by L2.  No LDS, no atomics, no scratch.  Every index is bounded
// before it is used: x < W, y < H; taps only on lanes that are in range, where 0 <= x0 <= W-2 and 0 <= y0 <= H-2 by
// construction.  Offsets are 64-bit.  The counts are sums of 0 / 1 decisions, each a function of the pixel and one other view:
// they are bit-reproducible and do not depend on the order of the other views.
#include "camera_device.h"

namespace mvip {
namespace depth_consistency {

namespace cam = mvip::camera;

__global__ __launch_bounds__(cam::TILE) void consistency_kernel(const float *__restrict__ disp, const float *__restrict__ pose,
                                                               const int V, const cam::PixelTiles s, const float focal32,
                                                               const float tol32, int *__restrict__ agree,
                                                               int *__restrict__ violated) {
    int n, x, y;
    if (!cam::tile_pixel(s, n, x, y)) return;
    const long long p = n * s.HW + (long long)y * s.W + x;
    const float d = disp[p];
    int n_agree = 0, n_violated = 0;
    if (cam::usable(d)) {
        const double focal = (double)focal32, tol = (double)tol32;
        double pw0, pw1, pw2;
        cam::unproject<double>(pose + (long long)n * 12, s.H, s.W, focal, x, y, 1.0 / (double)d, pw0, pw1, pw2);
        const double cu = (double)s.W * .5, cv = (double)s.H * .5;
        for (int src = 0; src < V; ++src) {
            if (src == n) continue;
            double u, v, ts;
            cam::project<double>(pose + (long long)src * 12, focal, cu, cv, pw0, pw1, pw2, u, v, ts);
            if (!cam::in_image(ts, u, v, s.H, s.W)) continue;
            int x0, y0;
            double fx, fy;
            cam::lower_footprint(u, v, s.H, s.W, x0, y0, fx, fy);
            const long long a = src * s.HW + (long long)y0 * s.W + x0, b = a + s.W;
            const float a00 = disp[a], a01 = disp[a + 1], a10 = disp[b], a11 = disp[b + 1];
            if (!(cam::usable(a00) && cam::usable(a01) && cam::usable(a10) && cam::usable(a11))) continue;
            const double ds = cam::lower_blend((double)a00, (double)a01, (double)a10, (double)a11, fx, fy);
            const double e = ts * ds - 1.0;
            if (fabs(e) <= tol) ++n_agree;
            else if (e < -tol) ++n_violated;
        }
    }
    agree[p] = n_agree;
    violated[p] = n_violated;
}

}  // namespace depth_consistency
}  // namespace mvip

using namespace mvip;

extern "C" int mvip_depth_consistency(const float *disp, const float *pose, int V, int H, int W, float focal, float tol,
                                      int *agree, int *violated, void *stream) {
    if (V < 0 || H < 2 || W < 2 || H > camera::MAX_SIDE || W > camera::MAX_SIDE) return MVIP_EINVAL;
    if (!camera::usable(focal) || !camera::usable(tol)) return MVIP_EINVAL;
    const camera::PixelTiles s = camera::make_tiles(H, W);
    if (V > INT32_MAX / s.T || V > INT32_MAX / 12) return MVIP_EINVAL;           // the grid, and n, fit an int
    if (V == 0) return MVIP_OK;
    if (!disp || !pose || !agree || !violated) return MVIP_EINVAL;
    hipLaunchKernelGGL(depth_consistency::consistency_kernel, dim3((unsigned)(V * s.T)), dim3(camera::TILE), 0, as_stream(stream),
                       disp, pose, V, s, focal, tol, agree, violated);
    return check_launch();
}
