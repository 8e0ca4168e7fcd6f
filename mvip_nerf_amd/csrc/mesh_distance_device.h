// The point-triangle distance and the shell walk over the face grid, shared by the closest-point query (csrc/mesh_distance.hip)
// and the signed distance (csrc/mesh_sdf.hip).  The definitions -- the four candidates and their order, the face grid, the
// margin, the stop rule -- are stated in the header of csrc/mesh_distance.hip; nothing here restates them differently.
//
// The arithmetic functions are __host__ __device__: tools/mesh_sdf_host_check.hip walks them on the host under the sanitizers.
//
// THE FEATURE CODE.  point_triangle also says which candidate supplied q: 0 the interior; for segment k (0: ab, 1: bc, 2: ca)
// with 0 < t < 1 the edge 1 + k; with t == 0 (ee == 0 included) the vertex 4 + k; with t == 1 the vertex 4 + (k + 1) % 3.
//
// THE BAND.  shell_walk takes cap2 (+inf: none) and stops once min(best, cap2) (1 + 2^-40) < L L: every face not yet met is
// then farther than both the best so far and the cap, so a face within the cap is never lost and the faces met within it are
// those of the walk without a cap.
#pragma once
#include "bitgrid_device.h"

namespace mvip {
namespace meshdist {

using namespace bitgrid;

constexpr double EPS = 1.0 / 2097152.0;                      // 2^-21
constexpr double STOP = 1.0 + 1.0 / 1099511627776.0;         // 1 + 2^-40

__host__ __device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// u x v
__host__ __device__ __forceinline__ void cross3(double ux, double uy, double uz, double vx, double vy, double vz, double &nx,
                                                double &ny, double &nz) {
    nx = uy * vz - uz * vy;
    ny = uz * vx - ux * vz;
    nz = ux * vy - uy * vx;
}

// segment k from u along e: replaces (d2, q, feat) where strictly nearer
__host__ __device__ __forceinline__ void segment(int k, double px, double py, double pz, double ux, double uy, double uz, double ex,
                                                 double ey, double ez, double &d2, double &qx, double &qy, double &qz, int &feat) {
    const double ee = dot3(ex, ey, ez, ex, ey, ez);
    double t = 0.0;
    if (ee > 0.0) {
        t = dot3(px - ux, py - uy, pz - uz, ex, ey, ez) / ee;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double sx = ux + t * ex, sy = uy + t * ey, sz = uz + t * ez;
    const double dx = px - sx, dy = py - sy, dz = pz - sz;
    const double s2 = dot3(dx, dy, dz, dx, dy, dz);
    if (s2 < d2) {
        d2 = s2;
        qx = sx;
        qy = sy;
        qz = sz;
        feat = t == 0.0 ? 4 + k : (t == 1.0 ? 4 + (k == 2 ? 0 : k + 1) : 1 + k);
    }
}

// POINT - TRIANGLE of csrc/mesh_distance.hip's header, with THE FEATURE CODE
__host__ __device__ __forceinline__ void point_triangle(double px, double py, double pz, double ax, double ay, double az, double bx,
                                                        double by, double bz, double cx, double cy, double cz, double &d2,
                                                        double &qx, double &qy, double &qz, int &feat) {
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
    const double cax = ax - cx, cay = ay - cy, caz = az - cz;
    double nx, ny, nz;
    cross3(abx, aby, abz, acx, acy, acz, nx, ny, nz);
    const double nn = dot3(nx, ny, nz, nx, ny, nz);
    d2 = __builtin_huge_val();
    qx = ax;
    qy = ay;
    qz = az;
    feat = 4;
    if (nn > 0.0) {
        const double apx = px - ax, apy = py - ay, apz = pz - az;
        double tx, ty, tz;
        cross3(abx, aby, abz, apx, apy, apz, tx, ty, tz);
        const double e0 = dot3(nx, ny, nz, tx, ty, tz);
        cross3(bcx, bcy, bcz, px - bx, py - by, pz - bz, tx, ty, tz);
        const double e1 = dot3(nx, ny, nz, tx, ty, tz);
        cross3(cax, cay, caz, px - cx, py - cy, pz - cz, tx, ty, tz);
        const double e2 = dot3(nx, ny, nz, tx, ty, tz);
        if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
            const double s = dot3(nx, ny, nz, apx, apy, apz);
            const double k = s / nn;
            d2 = s * s / nn;
            qx = px - nx * k;
            qy = py - ny * k;
            qz = pz - nz * k;
            feat = 0;
        }
    }
    segment(0, px, py, pz, ax, ay, az, abx, aby, abz, d2, qx, qy, qz, feat);
    segment(1, px, py, pz, bx, by, bz, bcx, bcy, bcz, d2, qx, qy, qz, feat);
    segment(2, px, py, pz, cx, cy, cz, cax, cay, caz, d2, qx, qy, qz, feat);
}

// face f against p, its vertices widened; false for an index outside [0, V)
__host__ __device__ __forceinline__ bool point_face(const float *__restrict__ verts, const int *__restrict__ faces, int V, int f,
                                                    double px, double py, double pz, double &d2, double &qx, double &qy, double &qz,
                                                    int &feat) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return false;
    point_triangle(px, py, pz, (double)verts[3 * a], (double)verts[3 * a + 1], (double)verts[3 * a + 2], (double)verts[3 * b],
                   (double)verts[3 * b + 1], (double)verts[3 * b + 2], (double)verts[3 * c], (double)verts[3 * c + 1],
                   (double)verts[3 * c + 2], d2, qx, qy, qz, feat);
    return true;
}

// clamp(g(x)) of the header for one axis
__host__ __device__ __forceinline__ int clamped_cell(float x, float o, float inv, int c) {
    const float f = floorf((x - o) * inv);
    return f >= (float)c ? c - 1 : (f >= 0.f ? (int)f : 0);      // NaN (never: the inputs are finite) would give 0
}

// THE QUERY of csrc/mesh_distance.hip's header for one finite point (fx, fy, fz), with THE BAND: on return best / bf / bq are
// the smallest d2, its face (-1: no face met) and its unrounded q among the faces met.  tests counts the point-face tests.
template <bool STATS>
__device__ __forceinline__ void shell_walk(float fx, float fy, float fz, const float *__restrict__ verts,
                                           const int *__restrict__ faces, int V, int F, const Grid &g, double wx, double wy,
                                           double wz, const int *__restrict__ cell_offsets, const int *__restrict__ cell_faces,
                                           double cap2, double &best, int &bf, double &bqx, double &bqy, double &bqz,
                                           unsigned &tests) {
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    const double ox = (double)g.bx, oy = (double)g.by, oz = (double)g.bz;
    const int ci = clamped_cell(fx, g.bx, g.ix, g.cx), cj = clamped_cell(fy, g.by, g.iy, g.cy),
              ck = clamped_cell(fz, g.bz, g.iz, g.cz);
    for (int r = 0;; ++r) {
        const int i0 = max(ci - r, 0), i1 = min(ci + r, g.cx - 1), j0 = max(cj - r, 0), j1 = min(cj + r, g.cy - 1),
                  k0 = max(ck - r, 0), k1 = min(ck + r, g.cz - 1);
        for (int i = i0; i <= i1; ++i) {
            const bool i_in = i > ci - r && i < ci + r;
            for (int j = j0; j <= j1; ++j) {
                const bool inner = i_in && j > cj - r && j < cj + r;      // only the two end cells of the row are new
                int k = inner ? (ck - r >= 0 ? ck - r : ck + r) : k0;
                while (k <= k1) {
                    const int l = (i * g.cy + j) * g.cz + k;
                    const int hi = cell_offsets[l + 1];
                    for (int u = cell_offsets[l]; u < hi; ++u) {
                        const int f = cell_faces[u];
                        if ((unsigned)f >= (unsigned)F) continue;                  // never: the grid is of this mesh
                        double d2, qx, qy, qz;
                        int feat;
                        if (!point_face(verts, faces, V, f, px, py, pz, d2, qx, qy, qz, feat)) continue;
                        if (STATS) ++tests;
                        if (d2 < best || (d2 == best && f < bf)) {
                            best = d2;
                            bf = f;
                            bqx = qx;
                            bqy = qy;
                            bqz = qz;
                        }
                    }
                    k = (inner && k < ck + r) ? ck + r : k + 1;
                }
            }
        }
        // the lower bound over the interior sides of the block
        double L = __builtin_huge_val();
        bool interior = false;
        if (ci - r >= 1) { interior = true; L = fmin(L, fmax(0.0, px - (ox + (double)(ci - r) * wx * (1.0 + EPS)))); }
        if (ci + r + 1 <= g.cx - 1) { interior = true; L = fmin(L, fmax(0.0, (ox + (double)(ci + r + 1) * wx * (1.0 - EPS)) - px)); }
        if (cj - r >= 1) { interior = true; L = fmin(L, fmax(0.0, py - (oy + (double)(cj - r) * wy * (1.0 + EPS)))); }
        if (cj + r + 1 <= g.cy - 1) { interior = true; L = fmin(L, fmax(0.0, (oy + (double)(cj + r + 1) * wy * (1.0 - EPS)) - py)); }
        if (ck - r >= 1) { interior = true; L = fmin(L, fmax(0.0, pz - (oz + (double)(ck - r) * wz * (1.0 + EPS)))); }
        if (ck + r + 1 <= g.cz - 1) { interior = true; L = fmin(L, fmax(0.0, (oz + (double)(ck + r + 1) * wz * (1.0 - EPS)) - pz)); }
        if (!interior || fmin(best, cap2) * STOP < L * L) break;
    }
}

}  // namespace meshdist
}  // namespace mvip
