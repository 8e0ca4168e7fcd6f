// TSDF fusion of rendered depth maps onto a lattice (beyond the reference: MVIP-NeRF has no mesh export and never fuses its
// depth renders; ops.tsdf_fuse, mesh.fuse_depths).  The zero level set of the fused field is the surface the renderer sees.
//
// Definition (the camera, its project and in_image, is csrc/camera_device.h's; the lattice is csrc/mcubes.hip's: point (i, j, k)
// sits at x0 + i hx, ..., hx = (x1 - x0) / (nx - 1) in fp32; tsdf / count [nx, ny, nz], z fastest; restated in
// tests/tsdf_numpy.py).  Per lattice point p, the views in ascending order, everything fp32 in this operation order:
//   acc = 0, cnt = 0
//   for v = 0 .. V-1:
//     (u, w, z) = project(pose_v, p)
//     xi = floor(u + .5), yi = floor(w + .5)        the nearest pixel: depth is not interpolated across discontinuities
//     skip unless z > 0, 0 <= xi <= W-1, 0 <= yi <= H-1        (in_image of the nearest pixel; a NaN fails every comparison)
//     skip if a mask is given and mask[v][yi][xi] == 0
//     d = disp[v][yi][xi];  skip unless d finite and > 0
//     sdf = 1/d - z;  skip if sdf < -trunc          (hidden behind the surface: not observed)
//     acc += min(1, sdf / trunc);  cnt += 1
//   tsdf = cnt > 0 ? acc / cnt : 1;  count = cnt
//
// Shape: a pure gather.  One thread per lattice point, lanes along z, a workgroup is 1,024 consecutive points; every point is
// written, so the outputs need no clearing.  The poses are read at wave-uniform addresses (into scalar registers); the mask
// byte and the disparity are gathered by the lanes that project inside the image, and the 64 points of a wave lie on one
// lattice line, so their pixels lie on one image line and the gathers are served by L2.  No LDS, no atomics, no scratch; the
// only loop runs over the V views.  Every index is bounded before it is used: n < N; xi, yi are compared as floats against
// [0, W-1] x [0, H-1] before the conversion.  Offsets are 64-bit.  A point's result depends on its own inputs only: a call
// equals its repetition bit for bit.
//
// Bytes from HBM: 8 written per lattice point; each view's 4 (5 with a mask) bytes per pixel at most once per pass of the
// lattice through the frustum, the gathers' repeats being served by L2 and the Infinity Cache (tools/tsdf_bench.py).
#include "camera_device.h"

namespace mvip {
namespace tsdf {

constexpr int BLOCK = 1024;

__global__ __launch_bounds__(BLOCK) void fuse_kernel(const float *__restrict__ disp, const float *__restrict__ pose,
                                                    const unsigned char *__restrict__ mask, const int V, const int H, const int W,
                                                    const float focal, const int ny, const int nz, const long long N, const float x0,
                                                    const float y0, const float z0, const float hx, const float hy, const float hz,
                                                    const float trunc, float *__restrict__ tsdf, int *__restrict__ count) {
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    const int k = (int)(n % nz), j = (int)((n / nz) % ny), i = (int)(n / ((long long)nz * ny));
    const float px = x0 + (float)i * hx, py = y0 + (float)j * hy, pz = z0 + (float)k * hz;
    const float cu = (float)W * .5f, cw = (float)H * .5f, umax = (float)(W - 1), wmax = (float)(H - 1);
    const long long HW = (long long)H * W;
    float acc = 0.f;
    int cnt = 0;
    for (int v = 0; v < V; ++v) {
        float u, w, z;
        camera::project<float>(pose + (long long)v * 12, focal, cu, cw, px, py, pz, u, w, z);
        const float fx = floorf(u + .5f), fy = floorf(w + .5f);
        // camera::in_image of the nearest pixel and camera::usable below, written out: through the calls the same tests compile
        // to another arrangement of this loop, measured 0.4 % slower
        if (!(z > 0.f && fx >= 0.f && fx <= umax && fy >= 0.f && fy <= wmax)) continue;
        const long long a = v * HW + (long long)(int)fy * W + (int)fx;      // 0 <= fx <= W-1, 0 <= fy <= H-1
        if (mask != nullptr && mask[a] == 0) continue;
        const float d = disp[a];
        if (!(d > 0.f && finite(d))) continue;
        const float sdf = 1.0f / d - z;
        if (sdf < -trunc) continue;
        acc += fminf(1.0f, sdf / trunc);
        ++cnt;
    }
    tsdf[n] = cnt > 0 ? acc / (float)cnt : 1.0f;
    count[n] = cnt;
}

}  // namespace tsdf
}  // namespace mvip

using namespace mvip;

constexpr int TSDF_MAX_AXIS = 768;

extern "C" int mvip_tsdf_fuse(const float *disp, const float *pose, const void *mask, int V, int H, int W, float focal, int nx,
                              int ny, int nz, float x0, float y0, float z0, float x1, float y1, float z1, float trunc,
                              float *tsdf_out, int *count, void *stream) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > TSDF_MAX_AXIS || ny > TSDF_MAX_AXIS || nz > TSDF_MAX_AXIS) return MVIP_EINVAL;
    if (V < 0 || H < 1 || W < 1 || H > camera::MAX_SIDE || W > camera::MAX_SIDE) return MVIP_EINVAL;
    if (!finite(x0) || !finite(y0) || !finite(z0) || !finite(x1) || !finite(y1) || !finite(z1) ||
        !(x0 < x1) || !(y0 < y1) || !(z0 < z1)) return MVIP_EINVAL;
    if (!camera::usable(focal) || !camera::usable(trunc)) return MVIP_EINVAL;
    if (!tsdf_out || !count || (V > 0 && (!disp || !pose))) return MVIP_EINVAL;
    const long long N = (long long)nx * ny * nz;
    const float hx = (x1 - x0) / (float)(nx - 1), hy = (y1 - y0) / (float)(ny - 1), hz = (z1 - z0) / (float)(nz - 1);
    hipLaunchKernelGGL(tsdf::fuse_kernel, dim3(blocks_for(N, tsdf::BLOCK)), dim3(tsdf::BLOCK), 0, as_stream(stream), disp, pose,
                       (const unsigned char *)mask, V, H, W, focal, ny, nz, N, x0, y0, z0, hx, hy, hz, trunc, tsdf_out, count);
    return check_launch();
}
