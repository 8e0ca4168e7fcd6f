// THE pinhole camera of the view-space kernels (warp.hip, depth_consistency.hip, tsdf.hip, raster.hip, texture.hip, rays.hip):
// one definition of how a pixel becomes a world point and a world point a pixel, restated for the tests in
// tests/camera_numpy.py.
//
// Conventions.  A pose is c2w [3, 4] row-major = [R | o], fp32.  The camera looks down -z.  There is no half-pixel offset: pixel
// (x, y) is the sample point u = x, v = y.  The ray parameter is the planar depth t, disparity = 1 / t:
//   unproject:  dx = (x - W .5) / f;  dy = -((y - H .5) / f);  p_c = (t dx, t dy, -t)
//               p_w[c] = ((p_c0 R[c][0] + p_c1 R[c][1]) + p_c2 R[c][2]) + o[c]
//   project:    dl = p - o;  q[j] = (R[0][j] dl0 + R[1][j] dl1) + R[2][j] dl2;  z = -q2
//               u = (f q0) / z + W .5;  v = -((f q1) / z) + H .5
// in the scalar T (float or double), the fp32 pose and the integers W, H widened to T first.  Every expression keeps this
// association and operand order (the library is built with -ffp-contract=off), so every kernel that calls these functions and
// the numpy restatement in the same precision compute the same bits.
#pragma once
#include "common.h"
#include <float.h>
#include <math.h>

namespace mvip {
namespace camera {

constexpr int MAX_SIDE = 16384;                  // the longest image side any view kernel takes

// finite and > 0: what a disparity, a focal length or a tolerance has to be to count; false for NaN
__host__ __device__ __forceinline__ bool usable(float v) { return v > 0.f && v <= FLT_MAX; }
__host__ __device__ __forceinline__ bool usable(double v) { return v > 0.0 && v <= DBL_MAX; }

// the camera-space direction (dx, dy, -1) of pixel (x, y), without its -1
template <class T>
__device__ __forceinline__ void pixel_dir(int x, int y, int H, int W, T f, T &dx, T &dy) {
    dx = ((T)x - (T)W * (T).5) / f;
    dy = -(((T)y - (T)H * (T).5) / f);
}

// the world point at planar depth t along the ray of pixel (x, y) of the camera P
template <class T>
__device__ __forceinline__ void unproject(const float *__restrict__ P, int H, int W, T f, int x, int y, T t, T &pw0, T &pw1, T &pw2) {
    T dx, dy;
    pixel_dir<T>(x, y, H, W, f, dx, dy);
    const T pc0 = t * dx, pc1 = t * dy, pc2 = -t;
    pw0 = ((pc0 * (T)P[0] + pc1 * (T)P[1]) + pc2 * (T)P[2]) + (T)P[3];
    pw1 = ((pc0 * (T)P[4] + pc1 * (T)P[5]) + pc2 * (T)P[6]) + (T)P[7];
    pw2 = ((pc0 * (T)P[8] + pc1 * (T)P[9]) + pc2 * (T)P[10]) + (T)P[11];
}

// the continuous image position (u, v) and the planar depth z of the world point (p0, p1, p2) in the camera P, with the image
// centre (cu, cv) = (W .5, H .5); nothing is tested here
template <class T>
__device__ __forceinline__ void project(const float *__restrict__ P, T f, T cu, T cv, T p0, T p1, T p2, T &u, T &v, T &z) {
    const T dl0 = p0 - (T)P[3], dl1 = p1 - (T)P[7], dl2 = p2 - (T)P[11];
    const T q0 = ((T)P[0] * dl0 + (T)P[4] * dl1) + (T)P[8] * dl2;
    const T q1 = ((T)P[1] * dl0 + (T)P[5] * dl1) + (T)P[9] * dl2;
    const T q2 = ((T)P[2] * dl0 + (T)P[6] * dl1) + (T)P[10] * dl2;
    z = -q2;
    u = (f * q0) / z + cu;
    v = -((f * q1) / z) + cv;
}

// in front of the camera and on the closed pixel lattice [0, W-1] x [0, H-1]; a NaN fails every comparison
template <class T>
__device__ __forceinline__ bool in_image(T z, T u, T v, int H, int W) {
    return z > (T)0 && u >= (T)0 && u <= (T)(W - 1) && v >= (T)0 && v <= (T)(H - 1);
}

// the bilinear footprint of an in_image position in an image of at least 2 x 2: the 2 x 2 pixels from (x0, y0), the LOWER
// corner clamped so that 0 <= x0 <= W-2 and 0 <= y0 <= H-2 (on the last column fx = 1), and the value there of four taps
template <class T>
__device__ __forceinline__ void lower_footprint(T u, T v, int H, int W, int &x0, int &y0, T &fx, T &fy) {
    x0 = min((int)floor(u), W - 2);
    y0 = min((int)floor(v), H - 2);
    fx = u - (T)x0;
    fy = v - (T)y0;
}

template <class T>
__device__ __forceinline__ T lower_blend(T a00, T a01, T a10, T a11, T fx, T fy) {
    const T gx = (T)1 - fx, gy = (T)1 - fy;
    const T top = a00 * gx + a01 * fx;
    const T bot = a10 * gx + a11 * fx;
    return top * gy + bot * fy;
}

// one thread per pixel of N images, lane = column: a workgroup is a tile of 64 columns x 4 rows, the grid N * T workgroups
constexpr int TX = 64, TY = 4, TILE = TX * TY;

struct PixelTiles {
    int H, W, tx, T;                             // tx tiles per row of tiles, T tiles per image
    long long HW;
};

static inline PixelTiles make_tiles(int H, int W) {
    const int tx = (W + TX - 1) / TX;
    return PixelTiles{H, W, tx, tx * ((H + TY - 1) / TY), (long long)H * W};
}

// this thread's image n and pixel (x, y); false where the tile overhangs the image
__device__ __forceinline__ bool tile_pixel(const PixelTiles &s, int &n, int &x, int &y) {
    n = blockIdx.x / s.T;
    const int tile = blockIdx.x % s.T;
    x = (tile % s.tx) * TX + lane_id();
    y = (tile / s.tx) * TY + (threadIdx.x >> 6);
    return x < s.W && y < s.H;
}

}  // namespace camera
}  // namespace mvip
