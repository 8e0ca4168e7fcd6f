// The per-view set-up of a face, shared by the mesh rasteriser (csrc/raster.hip) and the mesh texturing (csrc/texture.hip): ONE
// definition of the sub-pixel position of a vertex in a view (the projection itself is csrc/camera_device.h's, in fp64) and of
// the integer edge functions of a face there.  The definition is stated in the header comment of csrc/raster.hip (restated in
// tests/raster_numpy.py); every expression below keeps its association (the library is built with -ffp-contract=off), so both
// files compute the same bits.
#pragma once
#include "camera_device.h"

namespace mvip {
namespace raster {

constexpr int MAX_SIDE = camera::MAX_SIDE;
constexpr double BAND = 4194304.0;           // 2^22 sub-pixel units = 16,384 pixels

struct Camera {
    const float *P;                          // [3, 4] of this view
    double f, cu, cw, znear;
};

__device__ __forceinline__ bool project(const Camera &c, const float *__restrict__ verts, int i, int &X, int &Y, double &d) {
    const float *__restrict__ p = verts + 3 * (long long)i;
    double u, w, z;
    camera::project<double>(c.P, c.f, c.cu, c.cw, (double)p[0], (double)p[1], (double)p[2], u, w, z);
    d = 1.0 / z;
    const double su = 256.0 * u, sw = 256.0 * w;
    const bool ok = z >= c.znear && fabs(su) <= BAND && fabs(sw) <= BAND;      // a NaN fails
    X = ok ? (int)rint(su) : 0;                                                // |su|, |sw| <= 2^22 before the conversion
    Y = ok ? (int)rint(sw) : 0;
    return ok;
}

// a face set up for one view: A2 > 0 (vertices 1 and 2 swapped where it was negative)
struct Tri {
    int X0, Y0, X1, Y1, X2, Y2;
    double d0, d1, d2;
    long long A2;
    bool swapped;
};

// false: the face is dropped for this view.  i0, i1, i2 are inside [0, Nv).
__device__ __forceinline__ bool setup(const Camera &c, const float *__restrict__ verts, int i0, int i1, int i2, int cull, Tri &t) {
    bool ok = project(c, verts, i0, t.X0, t.Y0, t.d0);
    ok = project(c, verts, i1, t.X1, t.Y1, t.d1) && ok;
    ok = project(c, verts, i2, t.X2, t.Y2, t.d2) && ok;
    t.A2 = (long long)(t.X1 - t.X0) * (t.Y2 - t.Y0) - (long long)(t.Y1 - t.Y0) * (t.X2 - t.X0);
    t.swapped = t.A2 < 0;
    if (!ok || t.A2 == 0 || (cull && t.A2 > 0)) return false;
    if (t.swapped) {
        const int x = t.X1, y = t.Y1;
        const double d = t.d1;
        t.X1 = t.X2; t.Y1 = t.Y2; t.d1 = t.d2;
        t.X2 = x; t.Y2 = y; t.d2 = d;
        t.A2 = -t.A2;
    }
    return true;
}

// the three edge functions at pixel (x, y), their steps per pixel in x and y, and nb_k = 0 where edge k owns its zero, else 1
struct Edges {
    long long E0, E1, E2, dx0, dx1, dx2, dy0, dy1, dy2;
    int nb0, nb1, nb2;
};

__device__ __forceinline__ void edge(int Xi, int Yi, int Xj, int Yj, long long sx, long long sy, long long &E, long long &dx,
                                     long long &dy, int &nb) {
    const long long ex = Xj - Xi, ey = Yj - Yi;
    E = ex * (sy - Yi) - ey * (sx - Xi);
    dx = -256 * ey;
    dy = 256 * ex;
    nb = (ey < 0 || (ey == 0 && ex > 0)) ? 0 : 1;
}

__device__ __forceinline__ void edges_at(const Tri &t, int x, int y, Edges &e) {
    const long long sx = 256ll * x, sy = 256ll * y;
    edge(t.X1, t.Y1, t.X2, t.Y2, sx, sy, e.E0, e.dx0, e.dy0, e.nb0);
    edge(t.X2, t.Y2, t.X0, t.Y0, sx, sy, e.E1, e.dx1, e.dy1, e.nb1);
    edge(t.X0, t.Y0, t.X1, t.Y1, sx, sy, e.E2, e.dx2, e.dy2, e.nb2);
}

}  // namespace raster
}  // namespace mvip
