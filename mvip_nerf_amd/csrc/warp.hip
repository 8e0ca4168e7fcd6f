// Reference-view propagation: backward depth warping of source views into target views (beyond the reference, which has no
// counterpart: it reads RGB_inpainted/ as independent 2D inpaintings of every view; ops.warp_views, prepare.propagate_reference).
//
// Definition (conventions shared with tests/warp_numpy.py; the camera is get_rays', csrc/rays.hip: no half-pixel offset,
// c2w [3,4] row-major = [R | o], planar depth t, a camera-space point is t ((x - W/2)/f, -(y - H/2)/f, -1), disparity = 1/t).
// Per target n and pixel (y, x) whose mask byte is set and whose disparity is finite and > 0:
//   t = 1 / disp;  dx = (x - W .5) / f;  dy = -((y - H .5) / f);  p_c = (t dx, t dy, -t);
//   p_w[c] = ((p_c[0] R[c][0] + p_c[1] R[c][1]) + p_c[2] R[c][2]) + o[c]
//   for k = 0 .. S-1, s = order[n][k] (skipped unless 0 <= s < S), until a source is taken:
//     dl = p_w - o_s;  q[j] = (R_s[0][j] dl[0] + R_s[1][j] dl[1]) + R_s[2][j] dl[2];  t_s = -q[2]
//     u = (f q[0]) / t_s + W .5;  v = -((f q[1]) / t_s) + H .5
//     in range: t_s > 0, 0 <= u <= W-1, 0 <= v <= H-1   (a NaN fails every comparison)
//     x0 = min(floor(u), W-2), y0 = min(floor(v), H-2), fx = u - x0, fy = v - y0, gx = 1 - fx, gy = 1 - fy
//     a = (a[y0][x0] gx + a[y0][x0+1] fx) gy + (a[y0+1][x0] gx + a[y0+1][x0+1] fx) fy   for the source's disparity d_s and colour
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
#include "common.h"
#include <math.h>

namespace mvip {
namespace warp {

constexpr int TX = 64, TY = 4, BLOCK = TX * TY;
constexpr float FMAX = 3.402823466e38f;

struct Shape {
    int H, W, tx, T;                             // tx tiles per row of tiles, T tiles per image
    long long HW;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FMAX; }      // false for NaN

__device__ __forceinline__ float blend(float a00, float a01, float a10, float a11, float fx, float fy, float gx, float gy) {
    const float top = a00 * gx + a01 * fx;
    const float bot = a10 * gx + a11 * fx;
    return top * gy + bot * fy;
}

__global__ __launch_bounds__(BLOCK) void warp_kernel(const float *__restrict__ tgt_disp, const float *__restrict__ tgt_pose,
                                                    const unsigned char *__restrict__ tgt_mask, const Shape s,
                                                    const float *__restrict__ src_rgb, const float *__restrict__ src_disp,
                                                    const float *__restrict__ src_pose, const int S, const int *__restrict__ order,
                                                    const float focal, const float tol, float *__restrict__ rgb,
                                                    int *__restrict__ index, float *__restrict__ resid) {
    const int n = blockIdx.x / s.T, tile = blockIdx.x % s.T;
    const int x = (tile % s.tx) * TX + lane_id(), y = (tile / s.tx) * TY + (threadIdx.x >> 6);
    if (x >= s.W || y >= s.H) return;
    const long long p = n * s.HW + (long long)y * s.W + x;
    const float *__restrict__ P = tgt_pose + (long long)n * 12;
    const float d = tgt_disp[p];
    float out_r = 0.f, out_g = 0.f, out_b = 0.f, out_e = 0.f;
    int out_i = -1;
    if (tgt_mask[p] != 0 && d > 0.f && d <= FMAX) {
        const float t = 1.0f / d;
        const float dx = ((float)x - (float)s.W * .5f) / focal;
        const float dy = -(((float)y - (float)s.H * .5f) / focal);
        const float pc0 = t * dx, pc1 = t * dy, pc2 = -t;
        const float pw0 = ((pc0 * P[0] + pc1 * P[1]) + pc2 * P[2]) + P[3];
        const float pw1 = ((pc0 * P[4] + pc1 * P[5]) + pc2 * P[6]) + P[7];
        const float pw2 = ((pc0 * P[8] + pc1 * P[9]) + pc2 * P[10]) + P[11];
        const float umax = (float)(s.W - 1), vmax = (float)(s.H - 1);
        for (int k = 0; k < S && out_i < 0; ++k) {
            const int src = order[(long long)n * S + k];
            if (src < 0 || src >= S) continue;
            const float *__restrict__ Q = src_pose + (long long)src * 12;
            const float dl0 = pw0 - Q[3], dl1 = pw1 - Q[7], dl2 = pw2 - Q[11];
            const float q0 = (Q[0] * dl0 + Q[4] * dl1) + Q[8] * dl2;
            const float q1 = (Q[1] * dl0 + Q[5] * dl1) + Q[9] * dl2;
            const float q2 = (Q[2] * dl0 + Q[6] * dl1) + Q[10] * dl2;
            const float ts = -q2;
            const float u = (focal * q0) / ts + (float)s.W * .5f;
            const float v = -((focal * q1) / ts) + (float)s.H * .5f;
            if (!(ts > 0.f && u >= 0.f && u <= umax && v >= 0.f && v <= vmax)) continue;
            const int x0 = min((int)floorf(u), s.W - 2), y0 = min((int)floorf(v), s.H - 2);      // 0 <= x0 <= W-2, 0 <= y0 <= H-2
            const float fx = u - (float)x0, fy = v - (float)y0, gx = 1.0f - fx, gy = 1.0f - fy;
            const long long a = src * s.HW + (long long)y0 * s.W + x0, b = a + s.W;
            const float ds = blend(src_disp[a], src_disp[a + 1], src_disp[b], src_disp[b + 1], fx, fy, gx, gy);
            const float e = ts * ds - 1.0f;
            if (!(ds > 0.f && ds <= FMAX && fabsf(e) <= tol)) continue;
            const float *__restrict__ ca = src_rgb + a * 3, *__restrict__ cb = src_rgb + b * 3;
            const float r = blend(ca[0], ca[3], cb[0], cb[3], fx, fy, gx, gy);
            const float g = blend(ca[1], ca[4], cb[1], cb[4], fx, fy, gx, gy);
            const float bl = blend(ca[2], ca[5], cb[2], cb[5], fx, fy, gx, gy);
            if (!(finite_f(r) && finite_f(g) && finite_f(bl))) continue;
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

constexpr int WARP_MAX_SIDE = 16384;

extern "C" int mvip_warp_views(const float *tgt_disp, const float *tgt_pose, const void *tgt_mask, int64_t N, int H, int W,
                               const float *src_rgb, const float *src_disp, const float *src_pose, int S, const int *order,
                               float focal, float tol, float *rgb, int *index, float *resid, void *stream) {
    if (N < 0 || S < 0 || H < 2 || W < 2 || H > WARP_MAX_SIDE || W > WARP_MAX_SIDE) return MVIP_EINVAL;
    if (!(focal > 0.f) || !(focal <= warp::FMAX) || !(tol > 0.f) || !(tol <= warp::FMAX)) return MVIP_EINVAL;
    warp::Shape s;
    s.H = H;
    s.W = W;
    s.tx = (W + warp::TX - 1) / warp::TX;
    s.T = s.tx * ((H + warp::TY - 1) / warp::TY);
    s.HW = (long long)H * W;
    if (N > (int64_t)INT32_MAX / s.T || (int64_t)S > (int64_t)INT32_MAX / 12) return MVIP_EINVAL;      // the grid, and n, fit an int
    if (N == 0) return MVIP_OK;
    if (!tgt_disp || !tgt_pose || !tgt_mask || !rgb || !index || !resid) return MVIP_EINVAL;
    if (S > 0 && (!src_rgb || !src_disp || !src_pose || !order)) return MVIP_EINVAL;
    hipLaunchKernelGGL(warp::warp_kernel, dim3((unsigned)(N * s.T)), dim3(warp::BLOCK), 0, as_stream(stream), tgt_disp, tgt_pose,
                       (const unsigned char *)tgt_mask, s, src_rgb, src_disp, src_pose, S, order, focal, tol, rgb, index, resid);
    return check_launch();
}
