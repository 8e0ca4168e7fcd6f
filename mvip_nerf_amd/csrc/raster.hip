// Rasterisation of an indexed triangle mesh into the cameras it came from (beyond the reference: MVIP-NeRF has no mesh export
// and no rasteriser, so nothing here has a reference call site; ops.mesh_rasterize, mesh.render_views / visible_faces).  The
// inverse of prepare.render_disparities: per view the disparity map, the face-id map and the colour image the mesh presents,
// comparable pixel by pixel with the field's own renders.  THE statement of the definition; restated for the tests in
// tests/raster_numpy.py.  Everything is fp64 and integers (built with -ffp-contract=off; fp64 + - * / and rint are correctly
// rounded), so the restatement agrees BIT FOR BIT.
//
// The camera and its project are csrc/camera_device.h's, here with T = double; faces are counter-clockwise seen from outside
// (csrc/mcubes.hip).
//
// Per view, per vertex p (fp32 widened to fp64):
//   (u, w, z) = project(pose, p);  d = 1 / z
//   X = rint(256 u), Y = rint(256 w)                  8 sub-pixel bits, ties to even, integers from here on
// Per face: dropped whole for the view unless every vertex has z >= near and |256 u|, |256 w| <= 2^22 (compared in fp64 before
// the conversion; a NaN fails).  The bound is a guard band of 16,384 pixels (the largest image side), which keeps every edge
// function below 2^47: exact in int64 and in fp64.  THERE IS NO NEAR-PLANE CLIPPING: a face that straddles z = near vanishes.
//   A2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0)       x right, y down
//   A2 = 0: dropped.  A2 < 0: front-facing (the outside is towards the camera).  cull 'back' drops A2 > 0, 'none' keeps both.
//   When A2 < 0 vertices 1 and 2 are swapped (positions, d and colours), so that A2 > 0 from here on.
// Coverage of pixel (x, y), sx = 256 x, sy = 256 y: for the edge from vertex i to j opposite k (k = 0: 1 -> 2, k = 1: 2 -> 0,
// k = 2: 0 -> 1), E_k = (Xj - Xi)(sy - Yi) - (Yj - Yi)(sx - Xi); covered iff every E_k > 0, or E_k = 0 and the edge owns the
// pixel: with (ex, ey) = (Xj - Xi, Yj - Yi), ey < 0 or (ey = 0 and ex > 0).  That is the coverage of the sample point
// (x + eps, y + eps^2), the top-left rule; it does not depend on which face the edge belongs to, so two faces that share an edge
// never both cover a pixel and never both miss it.
// Fragment: D = fp32(((E0 d0 + E1 d1) + E2 d2) / A2) in fp64 (disparity is linear in screen space: the perspective-correct
// depth); skipped unless D is finite and > 0.
// Resolution: per pixel the largest 64-bit key (bits(D) << 32) | (0xFFFFFFFF - face) wins: the nearest fragment, the lower face
// index on equal disparity, whatever order the fragments arrive in.  disp = D of the winner (0 where none), face = its index
// (-1 where none); with colours, rgb = floor(c + .5) clamped to 0..255 of c = ((b0 c0 + b1 c1) + b2 c2) / ((b0 + b1) + b2),
// b_k = E_k d_k in fp64, recomputed for the winning face by the same arithmetic (0 where none).
//
// Shape.  Launch A (fragments): one thread per (face, view), 256 faces per workgroup.  The thread projects its face's three
// vertices itself (6x redundant fp64 work against a table of projected vertices per view, which for 2.5 M faces x 30 views
// would be 450 MB), sets up the integer edges and the bounding box clipped to the image.  A box of at most SMALL = 16 pixels is
// walked by its own thread.  Larger ones are walked by the whole wave afterwards: the lanes that hold one are balloted, the
// setup of each is broadcast in turn and the 64 lanes walk the box as 8 x 8 pixel tiles, so no thread ever loops alone over
// more than 16 pixels.  The edge functions are evaluated once per face and lane with multiplications and stepped in integers
// from there; the per-fragment fp64 work is the three products, two sums and one division of D.  Each covered, valid fragment
// costs one 8-byte load of the stored key and, only when its own key is larger, one no-return 64-bit atomicMax at device scope:
// the key only grows, so a stale read can only send an atomic that was not needed.  Launch B (resolve): one thread per pixel
// decodes the key; for colours it re-projects the winner's three vertices.  No LDS, no scratch, no float atomics; every launch
// on the caller's stream.  Every index is bounded before use: a face index outside [0, Nv) raises the flag and drops the face;
// the box is clamped to the image in integers that the guard band has bounded; offsets are 64-bit.
#include "common.h"
#include "raster_device.h"
#include <math.h>

namespace mvip {
namespace raster {

constexpr int BLOCK = 256;
constexpr int SMALL = 16;                    // the largest box, in pixels, that a thread walks alone
constexpr int64_t INT_MAX64 = 2147483647;

// one sample: the coverage test, D, the key, the early-out load and the atomic
template <bool STATS>
__device__ __forceinline__ void fragment(long long E0, long long E1, long long E2, int nb0, int nb1, int nb2, double d0, double d1,
                                         double d2, double A2, unsigned low, unsigned long long *addr, unsigned &n_frag,
                                         unsigned &n_sent) {
    if (((E0 - nb0) | (E1 - nb1) | (E2 - nb2)) < 0) return;
    const float D = (float)((((double)E0 * d0 + (double)E1 * d1) + (double)E2 * d2) / A2);
    if (!(D > 0.f && finite(D))) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(D) << 32) | low;
    if (STATS) ++n_frag;
    if (*addr >= key) return;                               // the key only grows: a stale value only costs an atomic
    if (STATS) ++n_sent;
    atomicMax(addr, key);                                   // no-return, device scope
}

template <bool STATS>
__global__ __launch_bounds__(BLOCK) void fragments_kernel(const float *__restrict__ verts, const int *__restrict__ faces, const int Nv,
                                                         const int F, const float *__restrict__ poses, const int blocks_per_view,
                                                         const int H, const int W, const double focal, const double znear,
                                                         const int cull, unsigned long long *keys, int *flag,
                                                         unsigned long long *stats) {
    const int v = blockIdx.x / blocks_per_view;
    const int fi = (blockIdx.x - v * blocks_per_view) * BLOCK + threadIdx.x;
    const Camera cam{poses + 12ll * v, focal, (double)W * 0.5, (double)H * 0.5, znear};
    unsigned long long *const view_keys = keys + (long long)v * H * W;
    unsigned n_frag = 0, n_sent = 0;

    Tri t{};
    int bx0 = 0, by0 = 0, bw = 0, bh = 0;
    bool valid = false;
    if (fi < F) {
        const int i0 = faces[3ll * fi], i1 = faces[3ll * fi + 1], i2 = faces[3ll * fi + 2];
        if ((unsigned)i0 >= (unsigned)Nv || (unsigned)i1 >= (unsigned)Nv || (unsigned)i2 >= (unsigned)Nv) {
            atomicOr(flag, 1);
        } else if (setup(cam, verts, i0, i1, i2, cull, t)) {
            // pixels x with 256 x inside [min X, max X], clamped to the image: integers within +-2^22, so no overflow
            const int xmin = min(t.X0, min(t.X1, t.X2)), xmax = max(t.X0, max(t.X1, t.X2));
            const int ymin = min(t.Y0, min(t.Y1, t.Y2)), ymax = max(t.Y0, max(t.Y1, t.Y2));
            bx0 = max(0, (xmin + 255) >> 8);
            by0 = max(0, (ymin + 255) >> 8);
            bw = min(W - 1, xmax >> 8) - bx0 + 1;
            bh = min(H - 1, ymax >> 8) - by0 + 1;
            valid = bw > 0 && bh > 0;
        }
    }
    const unsigned low = 0xFFFFFFFFu - (unsigned)fi;
    const bool large = valid && (long long)bw * bh > SMALL;

    if (valid && !large) {                                  // at most SMALL pixels, by this thread alone
        Edges e;
        edges_at(t, bx0, by0, e);
        const double A2 = (double)t.A2;
        for (int y = 0; y < bh; ++y) {
            long long E0 = e.E0, E1 = e.E1, E2 = e.E2;
            unsigned long long *row = view_keys + (long long)(by0 + y) * W + bx0;
            for (int x = 0; x < bw; ++x) {
                fragment<STATS>(E0, E1, E2, e.nb0, e.nb1, e.nb2, t.d0, t.d1, t.d2, A2, low, row + x, n_frag, n_sent);
                E0 += e.dx0; E1 += e.dx1; E2 += e.dx2;
            }
            e.E0 += e.dy0; e.E1 += e.dy1; e.E2 += e.dy2;
        }
    }

    // the large boxes, one after the other, by the whole wave: every lane of the wave arrives here
    unsigned long long pending = __ballot(large);
    const int lx = threadIdx.x & 7, ly = (threadIdx.x >> 3) & 7;
    while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        Tri s;
        s.X0 = __shfl(t.X0, src, 64); s.Y0 = __shfl(t.Y0, src, 64);
        s.X1 = __shfl(t.X1, src, 64); s.Y1 = __shfl(t.Y1, src, 64);
        s.X2 = __shfl(t.X2, src, 64); s.Y2 = __shfl(t.Y2, src, 64);
        s.d0 = __shfl(t.d0, src, 64); s.d1 = __shfl(t.d1, src, 64); s.d2 = __shfl(t.d2, src, 64);
        s.A2 = __shfl(t.A2, src, 64);
        const int sx0 = __shfl(bx0, src, 64), sy0 = __shfl(by0, src, 64), sw = __shfl(bw, src, 64), sh = __shfl(bh, src, 64);
        const unsigned slow = (unsigned)__shfl((int)low, src, 64);
        const double A2 = (double)s.A2;
        Edges e;
        edges_at(s, sx0 + lx, sy0 + ly, e);                 // this lane's pixel of the first tile; then steps of 8 pixels
        for (int ty = 0; ty < sh; ty += 8) {
            long long E0 = e.E0, E1 = e.E1, E2 = e.E2;
            const int y = ty + ly;
            unsigned long long *row = view_keys + (long long)(sy0 + y) * W + sx0;
            for (int tx = 0; tx < sw; tx += 8) {
                const int x = tx + lx;
                if (x < sw && y < sh)
                    fragment<STATS>(E0, E1, E2, e.nb0, e.nb1, e.nb2, s.d0, s.d1, s.d2, A2, slow, row + x, n_frag, n_sent);
                E0 += 8 * e.dx0; E1 += 8 * e.dx1; E2 += 8 * e.dx2;
            }
            e.E0 += 8 * e.dy0; e.E1 += 8 * e.dy1; e.E2 += 8 * e.dy2;
        }
    }
    if (STATS) {
        if (n_frag) atomicAdd(stats, (unsigned long long)n_frag);
        if (n_sent) atomicAdd(stats + 1, (unsigned long long)n_sent);
    }
}

__global__ __launch_bounds__(BLOCK) void clear_kernel(unsigned long long *__restrict__ keys, const long long N, int *flag,
                                                     unsigned long long *stats) {
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n < N) keys[n] = 0ull;
    if (n == 0) {
        *flag = 0;
        if (stats) stats[0] = stats[1] = 0ull;
    }
}

__global__ __launch_bounds__(BLOCK) void resolve_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ verts,
                                                       const int *__restrict__ faces, const unsigned char *__restrict__ colors,
                                                       const int Nv, const int F, const float *__restrict__ poses, const int H,
                                                       const int W, const long long N, const double focal, const double znear,
                                                       float *__restrict__ disp, int *__restrict__ face,
                                                       unsigned char *__restrict__ rgb) {
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    const unsigned long long key = keys[n];
    float D = 0.f;
    int fi = -1;
    unsigned char out[3] = {0, 0, 0};
    if (key != 0ull && 0xFFFFFFFFu - (unsigned)key < (unsigned)F) {
        fi = (int)(0xFFFFFFFFu - (unsigned)key);
        D = __uint_as_float((unsigned)(key >> 32));
        if (colors != nullptr) {
            const long long HW = (long long)H * W;
            const int v = (int)(n / HW);
            const int r = (int)(n - v * HW);
            const int y = r / W, x = r - y * W;
            const int i0 = faces[3ll * fi], i1 = faces[3ll * fi + 1], i2 = faces[3ll * fi + 2];
            const Camera cam{poses + 12ll * v, focal, (double)W * 0.5, (double)H * 0.5, znear};
            Tri t;
            if ((unsigned)i0 < (unsigned)Nv && (unsigned)i1 < (unsigned)Nv && (unsigned)i2 < (unsigned)Nv &&
                setup(cam, verts, i0, i1, i2, 0, t)) {
                Edges e;
                edges_at(t, x, y, e);
                const int j1 = t.swapped ? i2 : i1, j2 = t.swapped ? i1 : i2;
                const double b0 = (double)e.E0 * t.d0, b1 = (double)e.E1 * t.d1, b2 = (double)e.E2 * t.d2;
                const double den = (b0 + b1) + b2;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double c0 = (double)colors[3ll * i0 + ch], c1 = (double)colors[3ll * j1 + ch],
                                 c2 = (double)colors[3ll * j2 + ch];
                    const double c = ((b0 * c0 + b1 * c1) + b2 * c2) / den;
                    out[ch] = (unsigned char)(int)fmin(fmax(floor(c + 0.5), 0.0), 255.0);
                }
            }
        }
    }
    disp[n] = D;
    face[n] = fi;
    if (rgb != nullptr) {
        rgb[3 * n] = out[0];
        rgb[3 * n + 1] = out[1];
        rgb[3 * n + 2] = out[2];
    }
}

// the checks the two entry points share; N = the pixels of all views
static inline bool shape_ok(int64_t n_verts, int64_t n_faces, int64_t n_views, int H, int W, double focal, double znear,
                            long long &N) {
    if (n_verts < 0 || n_verts > INT_MAX64 || n_faces < 0 || 3 * n_faces > INT_MAX64 || n_views < 0 || n_views > INT_MAX64)
        return false;
    if (H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return false;
    if (!camera::usable(focal) || !camera::usable(znear)) return false;
    N = (long long)n_views * H * W;                         // < 2^31 * 2^28
    return (N + BLOCK - 1) / BLOCK <= INT_MAX64;
}

}  // namespace raster
}  // namespace mvip

using namespace mvip;
namespace rs = mvip::raster;

extern "C" int mvip_raster_fragments(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *poses,
                                     int64_t n_views, int H, int W, double focal, double znear, int cull, void *keys, int *flag,
                                     void *stats, void *stream) {
    long long N;
    if (!rs::shape_ok(n_verts, n_faces, n_views, H, W, focal, znear, N) || (cull != 0 && cull != 1)) return MVIP_EINVAL;
    const int64_t blocks_per_view = (n_faces + rs::BLOCK - 1) / rs::BLOCK;
    if (blocks_per_view * n_views > rs::INT_MAX64) return MVIP_EINVAL;
    if (!flag || (n_views > 0 && (!keys || !poses)) || (n_faces > 0 && !faces) || (n_verts > 0 && !verts)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(rs::clear_kernel, dim3(N > 0 ? blocks_for(N, rs::BLOCK) : 1u), dim3(rs::BLOCK), 0, s,
                       (unsigned long long *)keys, N, flag, (unsigned long long *)stats);
    if (n_views > 0 && n_faces > 0) {
        const dim3 grid((unsigned)(blocks_per_view * n_views)), block(rs::BLOCK);
        if (stats)
            hipLaunchKernelGGL(rs::fragments_kernel<true>, grid, block, 0, s, verts, faces, (int)n_verts, (int)n_faces, poses,
                               (int)blocks_per_view, H, W, focal, znear, cull, (unsigned long long *)keys, flag,
                               (unsigned long long *)stats);
        else
            hipLaunchKernelGGL(rs::fragments_kernel<false>, grid, block, 0, s, verts, faces, (int)n_verts, (int)n_faces, poses,
                               (int)blocks_per_view, H, W, focal, znear, cull, (unsigned long long *)keys, flag,
                               (unsigned long long *)nullptr);
    }
    return check_launch();
}

extern "C" int mvip_raster_resolve(const void *keys, const float *verts, const int *faces, const void *colors, int64_t n_verts,
                                   int64_t n_faces, const float *poses, int64_t n_views, int H, int W, double focal, double znear,
                                   float *disp, int *face, void *rgb, void *stream) {
    long long N;
    if (!rs::shape_ok(n_verts, n_faces, n_views, H, W, focal, znear, N)) return MVIP_EINVAL;
    if (rgb != nullptr && colors == nullptr && n_verts > 0) return MVIP_EINVAL;
    if ((n_views > 0 && (!keys || !poses || !disp || !face)) || (n_faces > 0 && !faces) || (n_verts > 0 && !verts)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    hipLaunchKernelGGL(rs::resolve_kernel, dim3(blocks_for(N, rs::BLOCK)), dim3(rs::BLOCK), 0, as_stream(stream),
                       (const unsigned long long *)keys, verts, faces, (const unsigned char *)colors, (int)n_verts, (int)n_faces,
                       poses, H, W, N, focal, znear, disp, face, (unsigned char *)rgb);
    return check_launch();
}
