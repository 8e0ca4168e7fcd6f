// Projective texturing of an indexed triangle mesh from the views it was built from (beyond the reference: MVIP-NeRF has no mesh
// export, so nothing here has a reference call site; ops.mesh_bake_points / mesh_bake_atlas / mesh_texture_resolve,
// mesh.bake_texture / colors_from_views / render_textured / save_obj).  A per-face texture atlas and per-point colours are baked
// from the images, with occlusion taken from the rasterised disparities of the same mesh (csrc/raster.hip), and the textured
// mesh is rendered back into any camera.  THE statement of the definition; restated for the tests in tests/texture_numpy.py.
// Everything is fp64 + - * /, floor and integers (built with -ffp-contract=off), so the restatement agrees BIT FOR BIT.
//
// ATLAS LAYOUT, a pure integer function of (F, n); n = texels along a face's leg, 1..32.
//   S = n + 3 the side of a block; faces 2k and 2k + 1 share block k; B = ceil(F / 2) blocks, row-major, Bx = the smallest
//   integer with Bx Bx >= B per row, By = ceil(B / Bx) rows (F = 0: Bx = By = 0).  Texture [Ht, Wt, 3] bytes, Wt = Bx S,
//   Ht = By S, both at most 16,384.
//   Texel (X, Y) (X along the row): bx = X div S, by = Y div S, k = by Bx + bx, (i, j) = (X - bx S, Y - by S).
//   i + j <= S - 1: owner = face 2k with (i, j).  Otherwise owner = face 2k + 1 with (i, j) <- (S - 1 - i, S - 1 - j).
//   An owner >= F is no owner (-1): the second half of the last block of an odd F, and the blocks past B; such texels hold 0.
//   The sample point of an owned texel, barycentrics over the face's vertices p0, p1, p2 (fp32 widened to fp64):
//     i + j <  n:  l1 = i / n, l2 = j / n, l0 = (1 - l1) - l2                                     the lattice inside the face
//     i + j >= n:  m = min(max(i - j + n, 0), 2 n), l1 = m / (2 n), l2 = (2 n - m) / (2 n), l0 = 0
//   The second rule is the texel's position projected at right angles onto the hypotenuse l1 + l2 = 1 (that is (i - j + n) / 2
//   along it, in integers over 2 n) and clamped to its end points.  On the hypotenuse itself (i + j = n) it gives l1 = i / n,
//   l2 = j / n again, with l0 exactly 0; in the gutter (i + j > n) it gives the nearest point of the CLOSED face, never an
//   extrapolated one, which would fail the visibility test.  The three corner texels (0, 0), (n, 0), (0, n) are p0, p1, p2.
//     p = (l0 p0 + l1 p1) + l2 p2 per coordinate in fp64, not rounded to fp32;  nrm = (p1 - p0) x (p2 - p0) in fp64:
//     nrm = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), e1 = p1 - p0, e2 = p2 - p0.
//   UV of the face's corners in continuous texel coordinates (texel centres at integer + 1/2): the lower half (face 2k) has
//   (bx S + 1/2 + n l1, by S + 1/2 + n l2), the upper half ((bx + 1) S - 1/2 - n l1, (by + 1) S - 1/2 - n l2).  A bilinear
//   lookup inside that triangle reaches texels of i + j <= n + 1 only; the lower half owns up to n + 2, the upper up to n + 1:
//   every texel of non-zero weight belongs to the face, and the owned sets are disjoint.
//
// BAKE of a sample point p with normal nrm (both fp64), views v = 0 .. V - 1 in ascending order.  View v contributes iff ALL of:
//   projection  (u, w, z) = camera::project<double> (camera_device.h: THE projection), z >= near
//   image       0 <= u <= W - 1 and 0 <= w <= H - 1
//   facing      l = o - p, c = (nrm0 l0 + nrm1 l1) + nrm2 l2; cull 'back': c > 0, 'none': c > 0 or c < 0
//   weight      nn = (nrm0^2 + nrm1^2) + nrm2^2 > 0, ll likewise, wgt = (c c) / (nn ll) finite and > 0    (cos^2 of incidence)
//   footprint   x0 = floor(u), x1 = min(x0 + 1, W - 1), fx = u - x0; y0, y1, fy likewise from w
//   visibility  at ALL FOUR pixels (x0|x1, y0|y1) the disparity D of the rasterised mesh is finite, > 0 and |D z - 1| <= tol
//   mask        with masks given (False = ignore), all four pixels True
//   A NaN anywhere fails.  A footprint that straddles an occlusion edge takes nothing from that view: intended.
//   colour per channel: top = c00 + fx (c10 - c00), bot = c01 + fx (c11 - c01), col = top + fy (bot - top), c_xy the byte at
//   (x_x, y_y) widened to fp64.
//   mode 'blend': rgb = floor((sum wgt col) / (sum wgt) + 1/2), the sums in view order;  mode 'best': floor(col + 1/2) of the
//   view of largest wgt, the lower index on a tie.  Clamped to 0..255.  wsum = fp32(sum wgt) (0: no view), best = that view or
//   -1; a point no view contributes to has rgb 0.
//
// TEXTURED RESOLVE of a face map [V, H, W] of the rasteriser: for face >= 0 the winner's set-up (raster::setup, cull off) and
//   b_k = E_k d_k, den = (b0 + b1) + b2 exactly as raster::resolve_kernel; la = b1 / den, lb = b2 / den belong to the set-up's
//   vertices 1 and 2, so (l1, l2) = swapped ? (lb, la) : (la, lb).  Sample position in texel-centre coordinates: lower half
//   sx = bx S + n l1, sy = by S + n l2; upper half sx = (bx S + S - 1) - n l1, sy = (by S + S - 1) - n l2.  With 0 <= sx <= Wt - 1
//   and 0 <= sy <= Ht - 1 (else 0): x0 = floor(sx), x1 = min(x0 + 1, Wt - 1), the bilinear formula above, floor(c + 1/2)
//   clamped.  0 where face < 0 or >= F, where a vertex index is out of range or the face is dropped for that view.
//
// Shape.  One thread per sample point, 256 per workgroup; the view loop is uniform across the wave, so the 12 pose floats of a
// view are wave-uniform loads.  The atlas instance derives face, barycentrics, point and normal from its texel index: nothing
// is materialised.  Texels map to lanes in texture row-major order (order 0) or block-major order (order 1: the S x S texels
// of a block are consecutive); both give the same texture.  No LDS, no atomics but the flag, no scratch; every launch on the
// caller's stream; every index is bounded before use and every offset is 64-bit.
#include "common.h"
#include "raster_device.h"
#include <float.h>
#include <math.h>

namespace mvip {
namespace texture {

namespace rs = mvip::raster;

constexpr int BLOCK = 256;
constexpr int MAX_TEXELS = 32;
constexpr int64_t INT_MAX64 = 2147483647;

struct Layout {
    int n, S, Bx, By, Wt, Ht;
};

// false: n outside 1..32, a negative F, or a texture side over 16,384
static inline bool make_layout(int64_t F, int n, Layout &L) {
    if (F < 0 || n < 1 || n > MAX_TEXELS) return false;
    const int S = n + 3;
    const int64_t B = (F + 1) / 2, most = rs::MAX_SIDE / S;
    int64_t bx = 0;
    while (bx * bx < B && bx <= most) ++bx;
    if (bx > most) return false;
    const int64_t by = bx ? (B + bx - 1) / bx : 0;            // <= bx
    L = Layout{n, S, (int)bx, (int)by, (int)(bx * S), (int)(by * S)};
    return true;
}

struct Views {
    const unsigned char *images;             // [V, H, W, 3]
    const float *disp;                       // [V, H, W]
    const unsigned char *masks;              // [V, H, W] or null
    const float *poses;                      // [V, 3, 4]
    int V, H, W;
    double f, znear, tol;
    int cull, mode;
};

__device__ __forceinline__ double bilinear(double c00, double c10, double c01, double c11, double fx, double fy) {
    const double top = c00 + fx * (c10 - c00), bot = c01 + fx * (c11 - c01);
    return top + fy * (bot - top);
}

__device__ __forceinline__ unsigned char to_byte(double c) { return (unsigned char)(int)fmin(fmax(floor(c + 0.5), 0.0), 255.0); }

// the bake of one sample point
__device__ __forceinline__ void bake(const Views &vw, const double p0, const double p1, const double p2, const double n0,
                                     const double n1, const double n2, unsigned char *__restrict__ rgb, float &wsum, int &best) {
    const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
    const long long HW = (long long)vw.H * vw.W;
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, bw = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    int bi = -1;
    for (int v = 0; v < vw.V; ++v) {
        const float *__restrict__ P = vw.poses + 12ll * v;
        double u, w, z;
        camera::project<double>(P, vw.f, (double)vw.W * 0.5, (double)vw.H * 0.5, p0, p1, p2, u, w, z);
        if (!(z >= vw.znear && u >= 0.0 && u <= (double)(vw.W - 1) && w >= 0.0 && w <= (double)(vw.H - 1))) continue;
        const double l0 = (double)P[3] - p0, l1 = (double)P[7] - p1, l2 = (double)P[11] - p2;
        const double c = (n0 * l0 + n1 * l1) + n2 * l2;
        if (!(vw.cull ? c > 0.0 : (c > 0.0 || c < 0.0))) continue;
        const double ll = (l0 * l0 + l1 * l1) + l2 * l2;
        const double wgt = (c * c) / (nn * ll);
        if (!(nn > 0.0 && wgt > 0.0 && wgt <= DBL_MAX)) continue;
        // the footprint clamps the UPPER corner (x1), so it also takes 1-pixel images: not camera::lower_footprint's rule
        const int x0 = (int)floor(u), y0 = (int)floor(w);                  // inside [0, W - 1] x [0, H - 1]
        const int x1 = min(x0 + 1, vw.W - 1), y1 = min(y0 + 1, vw.H - 1);
        const double fx = u - (double)x0, fy = w - (double)y0;
        const long long base = (long long)v * HW;
        const long long i00 = base + (long long)y0 * vw.W + x0, i10 = base + (long long)y0 * vw.W + x1;
        const long long i01 = base + (long long)y1 * vw.W + x0, i11 = base + (long long)y1 * vw.W + x1;
        const double D00 = (double)vw.disp[i00], D10 = (double)vw.disp[i10], D01 = (double)vw.disp[i01], D11 = (double)vw.disp[i11];
        bool ok = D00 > 0.0 && D00 <= DBL_MAX && fabs(D00 * z - 1.0) <= vw.tol;
        ok = ok && D10 > 0.0 && D10 <= DBL_MAX && fabs(D10 * z - 1.0) <= vw.tol;
        ok = ok && D01 > 0.0 && D01 <= DBL_MAX && fabs(D01 * z - 1.0) <= vw.tol;
        ok = ok && D11 > 0.0 && D11 <= DBL_MAX && fabs(D11 * z - 1.0) <= vw.tol;
        if (ok && vw.masks != nullptr) ok = vw.masks[i00] && vw.masks[i10] && vw.masks[i01] && vw.masks[i11];
        if (!ok) continue;
        const unsigned char *__restrict__ im = vw.images;
        const double c0 = bilinear((double)im[3 * i00], (double)im[3 * i10], (double)im[3 * i01], (double)im[3 * i11], fx, fy);
        const double c1 = bilinear((double)im[3 * i00 + 1], (double)im[3 * i10 + 1], (double)im[3 * i01 + 1], (double)im[3 * i11 + 1], fx, fy);
        const double c2 = bilinear((double)im[3 * i00 + 2], (double)im[3 * i10 + 2], (double)im[3 * i01 + 2], (double)im[3 * i11 + 2], fx, fy);
        sw += wgt;
        s0 += wgt * c0;
        s1 += wgt * c1;
        s2 += wgt * c2;
        if (wgt > bw) {                                                    // strictly: the lower view index keeps a tie
            bw = wgt; bi = v; b0 = c0; b1 = c1; b2 = c2;
        }
    }
    rgb[0] = rgb[1] = rgb[2] = 0;
    if (bi >= 0) {
        rgb[0] = to_byte(vw.mode ? b0 : s0 / sw);
        rgb[1] = to_byte(vw.mode ? b1 : s1 / sw);
        rgb[2] = to_byte(vw.mode ? b2 : s2 / sw);
    }
    wsum = (float)sw;
    best = bi;
}

__global__ __launch_bounds__(BLOCK) void bake_points_kernel(const float *__restrict__ points, const float *__restrict__ normals,
                                                           const long long N, const Views vw, unsigned char *__restrict__ rgb,
                                                           float *__restrict__ wsum, int *__restrict__ best) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= N) return;
    const float *__restrict__ p = points + 3 * t;
    const float *__restrict__ nr = normals + 3 * t;
    bake(vw, (double)p[0], (double)p[1], (double)p[2], (double)nr[0], (double)nr[1], (double)nr[2], rgb + 3 * t, wsum[t], best[t]);
}

template <int ORDER>
__global__ __launch_bounds__(BLOCK) void bake_atlas_kernel(const float *__restrict__ verts, const int *__restrict__ faces, const int Nv,
                                                          const int F, const Layout L, const Views vw, unsigned char *__restrict__ rgb,
                                                          float *__restrict__ wsum, int *__restrict__ best, int *flag) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long N = (long long)L.Wt * L.Ht;
    if (t >= N) return;
    int bx, by, i, j;
    if (ORDER == 0) {                                        // texture row-major
        const int Y = (int)(t / L.Wt), X = (int)(t - (long long)Y * L.Wt);
        bx = X / L.S; by = Y / L.S;
        i = X - bx * L.S; j = Y - by * L.S;
    } else {                                                 // block-major: the S x S texels of a block are consecutive
        const int SS = L.S * L.S;
        const int blk = (int)(t / SS), r = (int)(t - (long long)blk * SS);
        by = blk / L.Bx; bx = blk - by * L.Bx;
        j = r / L.S; i = r - j * L.S;
    }
    const long long out = ((long long)by * L.S + j) * L.Wt + ((long long)bx * L.S + i);
    long long fi = 2 * ((long long)by * L.Bx + bx);
    if (i + j > L.S - 1) {
        i = L.S - 1 - i; j = L.S - 1 - j;
        ++fi;
    }
    unsigned char c[3] = {0, 0, 0};
    float ws = 0.f;
    int bi = -1;
    if (fi < F) {
        const int i0 = faces[3 * fi], i1 = faces[3 * fi + 1], i2 = faces[3 * fi + 2];
        if ((unsigned)i0 >= (unsigned)Nv || (unsigned)i1 >= (unsigned)Nv || (unsigned)i2 >= (unsigned)Nv) {
            atomicOr(flag, 1);
        } else {
            const int n = L.n;
            double l0, l1, l2;
            if (i + j < n) {
                l1 = (double)i / (double)n;
                l2 = (double)j / (double)n;
                l0 = (1.0 - l1) - l2;
            } else {
                const int m = min(max(i - j + n, 0), 2 * n);
                l1 = (double)m / (double)(2 * n);
                l2 = (double)(2 * n - m) / (double)(2 * n);
                l0 = 0.0;
            }
            const float *__restrict__ q0 = verts + 3ll * i0;
            const float *__restrict__ q1 = verts + 3ll * i1;
            const float *__restrict__ q2 = verts + 3ll * i2;
            const double x0 = q0[0], y0 = q0[1], z0 = q0[2], x1 = q1[0], y1 = q1[1], z1 = q1[2], x2 = q2[0], y2 = q2[1], z2 = q2[2];
            const double px = (l0 * x0 + l1 * x1) + l2 * x2, py = (l0 * y0 + l1 * y1) + l2 * y2, pz = (l0 * z0 + l1 * z1) + l2 * z2;
            const double e1x = x1 - x0, e1y = y1 - y0, e1z = z1 - z0, e2x = x2 - x0, e2y = y2 - y0, e2z = z2 - z0;
            const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            bake(vw, px, py, pz, nx, ny, nz, c, ws, bi);
        }
    }
    rgb[3 * out] = c[0];
    rgb[3 * out + 1] = c[1];
    rgb[3 * out + 2] = c[2];
    wsum[out] = ws;
    best[out] = bi;
}

__global__ __launch_bounds__(BLOCK) void resolve_kernel(const int *__restrict__ face, const float *__restrict__ verts,
                                                       const int *__restrict__ faces, const int Nv, const int F,
                                                       const unsigned char *__restrict__ atlas, const Layout L,
                                                       const float *__restrict__ poses, const int H, const int W, const long long N,
                                                       const double focal, const double znear, unsigned char *__restrict__ rgb) {
    const long long n = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (n >= N) return;
    const int fi = face[n];
    unsigned char out[3] = {0, 0, 0};
    if (fi >= 0 && fi < F) {
        const long long HW = (long long)H * W;
        const int v = (int)(n / HW);
        const int r = (int)(n - v * HW);
        const int y = r / W, x = r - y * W;
        const int i0 = faces[3ll * fi], i1 = faces[3ll * fi + 1], i2 = faces[3ll * fi + 2];
        const rs::Camera cam{poses + 12ll * v, focal, (double)W * 0.5, (double)H * 0.5, znear};
        rs::Tri t;
        if ((unsigned)i0 < (unsigned)Nv && (unsigned)i1 < (unsigned)Nv && (unsigned)i2 < (unsigned)Nv &&
            rs::setup(cam, verts, i0, i1, i2, 0, t)) {
            rs::Edges e;
            rs::edges_at(t, x, y, e);
            const double b0 = (double)e.E0 * t.d0, b1 = (double)e.E1 * t.d1, b2 = (double)e.E2 * t.d2;
            const double den = (b0 + b1) + b2;
            const double la = b1 / den, lb = b2 / den;
            const double l1 = t.swapped ? lb : la, l2 = t.swapped ? la : lb;
            const int k = fi >> 1;
            const int by = k / L.Bx, bx = k - by * L.Bx;
            const double dn = (double)L.n;
            const double sx = (fi & 1) ? (double)(bx * L.S + L.S - 1) - dn * l1 : (double)(bx * L.S) + dn * l1;
            const double sy = (fi & 1) ? (double)(by * L.S + L.S - 1) - dn * l2 : (double)(by * L.S) + dn * l2;
            if (sx >= 0.0 && sx <= (double)(L.Wt - 1) && sy >= 0.0 && sy <= (double)(L.Ht - 1)) {   // a NaN fails
                const int x0 = (int)floor(sx), y0 = (int)floor(sy);
                const int x1 = min(x0 + 1, L.Wt - 1), y1 = min(y0 + 1, L.Ht - 1);
                const double fx = sx - (double)x0, fy = sy - (double)y0;
                const long long j00 = 3 * ((long long)y0 * L.Wt + x0), j10 = 3 * ((long long)y0 * L.Wt + x1);
                const long long j01 = 3 * ((long long)y1 * L.Wt + x0), j11 = 3 * ((long long)y1 * L.Wt + x1);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    out[ch] = to_byte(bilinear((double)atlas[j00 + ch], (double)atlas[j10 + ch], (double)atlas[j01 + ch],
                                               (double)atlas[j11 + ch], fx, fy));
            }
        }
    }
    rgb[3 * n] = out[0];
    rgb[3 * n + 1] = out[1];
    rgb[3 * n + 2] = out[2];
}

// the checks of the cameras and images that the entry points share
static inline bool views_ok(int64_t n_views, int H, int W, double focal, double znear) {
    if (n_views < 0 || n_views > INT_MAX64) return false;
    if (H < 1 || W < 1 || H > rs::MAX_SIDE || W > rs::MAX_SIDE) return false;
    return camera::usable(focal) && camera::usable(znear);
}

static inline bool bake_ok(int64_t n_views, int H, int W, double focal, double znear, double tol, int cull, int mode) {
    return views_ok(n_views, H, W, focal, znear) && tol >= 0.0 && tol <= DBL_MAX && (cull == 0 || cull == 1) && (mode == 0 || mode == 1);
}

}  // namespace texture
}  // namespace mvip

using namespace mvip;
namespace tx = mvip::texture;

extern "C" int mvip_texture_bake_points(const float *points, const float *normals, int64_t n_points, const void *images,
                                        const float *disp, const void *masks, const float *poses, int64_t n_views, int H, int W,
                                        double focal, double znear, double tol, int cull, int mode, void *rgb, float *wsum,
                                        int *best, void *stream) {
    if (!tx::bake_ok(n_views, H, W, focal, znear, tol, cull, mode)) return MVIP_EINVAL;
    if (n_points < 0 || (n_points + tx::BLOCK - 1) / tx::BLOCK > tx::INT_MAX64) return MVIP_EINVAL;
    if (n_points > 0 && (!points || !normals || !rgb || !wsum || !best)) return MVIP_EINVAL;
    if (n_views > 0 && (!images || !disp || !poses)) return MVIP_EINVAL;
    if (n_points == 0) return MVIP_OK;
    const tx::Views vw{(const unsigned char *)images, disp, (const unsigned char *)masks, poses, (int)n_views, H, W, focal, znear, tol, cull, mode};
    hipLaunchKernelGGL(tx::bake_points_kernel, dim3(blocks_for(n_points, tx::BLOCK)), dim3(tx::BLOCK), 0, as_stream(stream), points,
                       normals, (long long)n_points, vw, (unsigned char *)rgb, wsum, best);
    return check_launch();
}

extern "C" int mvip_texture_bake_atlas(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, int texels, int order,
                                       const void *images, const float *disp, const void *masks, const float *poses,
                                       int64_t n_views, int H, int W, double focal, double znear, double tol, int cull, int mode,
                                       void *rgb, float *wsum, int *best, int *flag, void *stream) {
    tx::Layout L;
    if (!tx::bake_ok(n_views, H, W, focal, znear, tol, cull, mode)) return MVIP_EINVAL;
    if (n_verts < 0 || n_verts > tx::INT_MAX64 || n_faces < 0 || 3 * n_faces > tx::INT_MAX64) return MVIP_EINVAL;
    if (!tx::make_layout(n_faces, texels, L) || (order != 0 && order != 1)) return MVIP_EINVAL;
    if (!flag || (n_faces > 0 && (!faces || !rgb || !wsum || !best)) || (n_verts > 0 && !verts)) return MVIP_EINVAL;
    if (n_views > 0 && (!images || !disp || !poses)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    zero_words(flag, 1, s);
    const long long N = (long long)L.Wt * L.Ht;              // <= 2^28
    if (N > 0) {
        const tx::Views vw{(const unsigned char *)images, disp, (const unsigned char *)masks, poses, (int)n_views, H, W, focal, znear, tol, cull, mode};
        const dim3 grid(blocks_for(N, tx::BLOCK)), block(tx::BLOCK);
        if (order == 0)
            hipLaunchKernelGGL(tx::bake_atlas_kernel<0>, grid, block, 0, s, verts, faces, (int)n_verts, (int)n_faces, L, vw,
                               (unsigned char *)rgb, wsum, best, flag);
        else
            hipLaunchKernelGGL(tx::bake_atlas_kernel<1>, grid, block, 0, s, verts, faces, (int)n_verts, (int)n_faces, L, vw,
                               (unsigned char *)rgb, wsum, best, flag);
    }
    return check_launch();
}

extern "C" int mvip_texture_resolve(const int *face, const float *verts, const int *faces, int64_t n_verts, int64_t n_faces,
                                    const void *atlas, int texels, const float *poses, int64_t n_views, int H, int W, double focal,
                                    double znear, void *rgb, void *stream) {
    tx::Layout L;
    if (!tx::views_ok(n_views, H, W, focal, znear)) return MVIP_EINVAL;
    if (n_verts < 0 || n_verts > tx::INT_MAX64 || n_faces < 0 || 3 * n_faces > tx::INT_MAX64) return MVIP_EINVAL;
    if (!tx::make_layout(n_faces, texels, L)) return MVIP_EINVAL;
    const long long N = (long long)n_views * H * W;
    if ((N + tx::BLOCK - 1) / tx::BLOCK > tx::INT_MAX64) return MVIP_EINVAL;
    if ((n_views > 0 && (!face || !poses || !rgb)) || (n_faces > 0 && (!faces || !atlas)) || (n_verts > 0 && !verts)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    hipLaunchKernelGGL(tx::resolve_kernel, dim3(blocks_for(N, tx::BLOCK)), dim3(tx::BLOCK), 0, as_stream(stream), face, verts, faces,
                       (int)n_verts, (int)n_faces, (const unsigned char *)atlas, L, poses, H, W, N, focal, znear,
                       (unsigned char *)rgb);
    return check_launch();
}
