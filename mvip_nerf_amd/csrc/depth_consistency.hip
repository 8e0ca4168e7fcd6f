// Cross-view depth consistency: per pixel of every view, how many other views see a surface at the same place (agreement) and
// how many see THROUGH that place to something farther (a free-space violation, the signature of a floater).  Beyond the
// reference, which has no counterpart (ops.depth_consistency, prepare.consistency_mask).
//
// Definition, in fp64 on the fp32 inputs (the conventions are mvip_warp_views' / mvip_tsdf_fuse's: c2w [3,4] row-major = [R | o],
// no half-pixel offset, cameras look down -z, disparity = 1 / planar depth; the expressions and their association are those of
// tests/warp_numpy.py::warp with dtype=np.float64, restated in tests/depth_consistency_numpy.py).  A target is a pixel (y, x) of
// view n whose disparity d is finite and > 0:
//   t = 1 / d;  dx = (x - W .5) / f;  dy = -((y - H .5) / f);  p_c = (t dx, t dy, -t)
//   p_w[c] = ((p_c[0] R[c][0] + p_c[1] R[c][1]) + p_c[2] R[c][2]) + o[c]
//   for every view s != n, in ascending s:
//     dl = p_w - o_s;  q[j] = (R_s[0][j] dl[0] + R_s[1][j] dl[1]) + R_s[2][j] dl[2];  t_s = -q[2]
//     u = (f q[0]) / t_s + W .5;  v = -((f q[1]) / t_s) + H .5
//     in range: t_s > 0, 0 <= u <= W-1, 0 <= v <= H-1   (a NaN fails every comparison)
//     x0 = min(floor(u), W-2), y0 = min(floor(v), H-2), fx = u - x0, fy = v - y0, gx = 1 - fx, gy = 1 - fy
//     valid: ALL FOUR taps of view s's disparity finite and > 0 (the four-pixel rule of csrc/texture.hip: a caller masks a pixel
//            by zeroing it)
//     d_s = (a[y0][x0] gx + a[y0][x0+1] fx) gy + (a[y0+1][x0] gx + a[y0+1][x0+1] fx) fy;  resid = t_s d_s - 1
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
#include "common.h"
#include <math.h>

namespace mvip {
namespace depth_consistency {

constexpr int TX = 64, TY = 4, BLOCK = TX * TY;
constexpr int MAX_SIDE = 16384;
constexpr float FMAX = 3.402823466e38f;

struct Shape {
    int H, W, tx, T;                             // tx tiles per row of tiles, T tiles per image
    long long HW;
};

__device__ __forceinline__ bool usable(float d) { return d > 0.f && d <= FMAX; }      // finite and > 0; false for NaN

__global__ __launch_bounds__(BLOCK) void consistency_kernel(const float *__restrict__ disp, const float *__restrict__ pose,
                                                           const int V, const Shape s, const float focal32, const float tol32,
                                                           int *__restrict__ agree, int *__restrict__ violated) {
    const int n = blockIdx.x / s.T, tile = blockIdx.x % s.T;
    const int x = (tile % s.tx) * TX + lane_id(), y = (tile / s.tx) * TY + (threadIdx.x >> 6);
    if (x >= s.W || y >= s.H) return;
    const long long p = n * s.HW + (long long)y * s.W + x;
    const float d = disp[p];
    int n_agree = 0, n_violated = 0;
    if (usable(d)) {
        const double focal = (double)focal32, tol = (double)tol32;
        const float *__restrict__ P = pose + (long long)n * 12;
        const double t = 1.0 / (double)d;
        const double dx = ((double)x - (double)s.W * .5) / focal;
        const double dy = -(((double)y - (double)s.H * .5) / focal);
        const double pc0 = t * dx, pc1 = t * dy, pc2 = -t;
        const double pw0 = ((pc0 * (double)P[0] + pc1 * (double)P[1]) + pc2 * (double)P[2]) + (double)P[3];
        const double pw1 = ((pc0 * (double)P[4] + pc1 * (double)P[5]) + pc2 * (double)P[6]) + (double)P[7];
        const double pw2 = ((pc0 * (double)P[8] + pc1 * (double)P[9]) + pc2 * (double)P[10]) + (double)P[11];
        const double umax = (double)(s.W - 1), vmax = (double)(s.H - 1);
        for (int src = 0; src < V; ++src) {
            if (src == n) continue;
            const float *__restrict__ Q = pose + (long long)src * 12;
            const double dl0 = pw0 - (double)Q[3], dl1 = pw1 - (double)Q[7], dl2 = pw2 - (double)Q[11];
            const double q0 = ((double)Q[0] * dl0 + (double)Q[4] * dl1) + (double)Q[8] * dl2;
            const double q1 = ((double)Q[1] * dl0 + (double)Q[5] * dl1) + (double)Q[9] * dl2;
            const double q2 = ((double)Q[2] * dl0 + (double)Q[6] * dl1) + (double)Q[10] * dl2;
            const double ts = -q2;
            const double u = (focal * q0) / ts + (double)s.W * .5;
            const double v = -((focal * q1) / ts) + (double)s.H * .5;
            if (!(ts > 0.0 && u >= 0.0 && u <= umax && v >= 0.0 && v <= vmax)) continue;
            const int x0 = min((int)floor(u), s.W - 2), y0 = min((int)floor(v), s.H - 2);      // 0 <= x0 <= W-2, 0 <= y0 <= H-2
            const long long a = src * s.HW + (long long)y0 * s.W + x0, b = a + s.W;
            const float a00 = disp[a], a01 = disp[a + 1], a10 = disp[b], a11 = disp[b + 1];
            if (!(usable(a00) && usable(a01) && usable(a10) && usable(a11))) continue;
            const double fx = u - (double)x0, fy = v - (double)y0, gx = 1.0 - fx, gy = 1.0 - fy;
            const double top = (double)a00 * gx + (double)a01 * fx;
            const double bot = (double)a10 * gx + (double)a11 * fx;
            const double ds = top * gy + bot * fy;
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
    namespace dc = depth_consistency;
    if (V < 0 || H < 2 || W < 2 || H > dc::MAX_SIDE || W > dc::MAX_SIDE) return MVIP_EINVAL;
    if (!(focal > 0.f) || !(focal <= dc::FMAX) || !(tol > 0.f) || !(tol <= dc::FMAX)) return MVIP_EINVAL;
    dc::Shape s;
    s.H = H;
    s.W = W;
    s.tx = (W + dc::TX - 1) / dc::TX;
    s.T = s.tx * ((H + dc::TY - 1) / dc::TY);
    s.HW = (long long)H * W;
    if (V > INT32_MAX / s.T || V > INT32_MAX / 12) return MVIP_EINVAL;           // the grid, and n, fit an int
    if (V == 0) return MVIP_OK;
    if (!disp || !pose || !agree || !violated) return MVIP_EINVAL;
    hipLaunchKernelGGL(dc::consistency_kernel, dim3((unsigned)(V * s.T)), dim3(dc::BLOCK), 0, as_stream(stream), disp, pose, V, s,
                       focal, tol, agree, violated);
    return check_launch();
}
