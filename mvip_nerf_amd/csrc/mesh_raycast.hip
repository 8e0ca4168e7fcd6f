// Mesh ray casting (beyond the reference, which has no mesh export at all): the first face of an indexed triangle mesh that
// each of N rays hits, occlusion ("any hit"), and per face the number of directions in which it sees nothing (ops.mesh_cast_rays
// / mesh_occluded / mesh_face_openness, mesh.cast_rays / cast_views / face_openness / drop_interior), on the face grid of
// csrc/mesh_distance.hip.  THE statement of the definitions; restated for the tests in tests/mesh_raycast_numpy.py.
//
// verts [V, 3] fp32, faces [F, 3] int32.  A ray is (o[3], d[3], tmin, tmax) in fp32 (the openness sweep uses its fp64 centroids
// as origins).  All arithmetic is fp64 on the widened inputs, every expression associates as written (the library is built with
// -ffp-contract=off).
//
// RAY - TRIANGLE, the watertight test of Woop, Benthin, Wald 2013 ("Watertight Ray/Triangle Intersection", JCGT 2(1)):
//   kz = the axis of largest |d|, the lowest axis among equals; kx, ky the next two axes cyclically, swapped when d[kz] < 0;
//   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];
//   a vertex P becomes A = P - o, Px = A[kx] - Sx A[kz], Py = A[ky] - Sy A[kz], Pz = Sz A[kz];
//   with (A, B, C) the transformed vertices: U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax;
//   the face is a candidate iff all three are >= 0 or all three are <= 0 (no culling); det = (U + V) + W must be non-zero;
//   t = ((U Az + V Bz) + W Cz) / det; the face is hit iff tmin <= t <= tmax.
// An edge function depends only on the two transformed vertices of its edge, and a vertex transforms the same way whichever
// face it belongs to: the two faces on an edge see exactly opposite signs, so no ray passes between them.  A face that names
// a vertex twice has V (or U, or W) == 0 and the other two exactly opposite: det == 0, never hit.
//
// RESULT.  The hit of smallest fp64 t, the lowest face index among equals, the face skip[n] (-1: none) never counting:
// face int32 (-1: a miss), t = fp32(t) (+inf: a miss), bary = (fp32(V / det), fp32(W / det)), the weights of the second and
// third vertex (NaN without a hit).  An INVALID ray -- o or d with a NaN or infinite component, d = 0, tmin not finite, tmax NaN
// or < tmin; tmax = +inf is allowed -- gives face -1 and t NaN and never enters the traversal.  OCCLUSION is face >= 0 of the
// same definition; the any-hit kernel stops at the first accepted hit and returns that face.  THE RESULT DOES NOT DEPEND ON THE
// GRID below; the grid only decides which faces are tested.
//
// FACE OPENNESS.  Per face f and direction d_k [K, 3] fp32, K <= 255: origin = the centroid ((a + b) + c) / 3 in fp64,
// N = (b - a) x (c - a); d_k is on the front side iff N . d_k > 0, on the back side iff < 0, skipped iff == 0
// (N . d = (N0 d0 + N1 d1) + N2 d2); it is OPEN iff the ray (centroid, d_k, 0, max_dist) hits nothing with skip = f.  Counts
// [4, F] int32: front_open, front_total, back_open, back_total.  One thread per face loops over K; nothing of size F K exists.
//
// THE TRAVERSAL, one thread per ray, on the FaceGrid of csrc/mesh_distance.hip (its header: lo(k) = og + k w (1 + EPS) and
// hi(k) = og + k w (1 - EPS), EPS = 2^-21, w = 1 / inv; a face whose cell range on an axis is [r0, r1] lies wholly inside
// (hi(r0), lo(r1 + 1)), the ends at the grid boundary being open outwards because cell indices are clamped).  Write D(k) =
// [hi(k) - s, lo(k + 1) + s] for the DILATED SLAB of cell k on an axis, with D(0) open below and D(c - 1) open above, and s the
// ray's slack (below).  Claim: a face f whose test accepts the ray at parameter t* <= best is tested.
//   The point X* = o + t* d lies within s / 2 of f's bounding box on every axis (THE SLACK below).  So on every axis some k of
//   f's cell range has X*_a in D_a(k) with s / 2 to spare, and f is in the list of the cell made of those three k.
//   1. The ray is cut to [t0, t1] = [tmin, tmax] intersected, per axis, with the parameters at which it is inside
//      [bmin_a - s, bmax_a + s], bmin / bmax the fp32 bounds of the mesh's vertices (an axis with d_a == 0 is a test of o_a); an
//      empty interval is a miss.  t* is inside: X* is within s / 2 of a box inside the bounds.
//   2. m = the axis of largest |d_a| inv_a (the lowest among equals; d_m != 0).  The cells k0 .. k1 of m whose dilated slab
//      meets the ray's coordinate range over [t0, t1] are walked in ray order -- at most cells[m] <= 512 slabs.
//   3. Per slab k: [ta, tb] = [t0, min(t1, best)] cut to the parameters at which the ray is in D_m(k).  It holds t* for the k
//      above.  On each other axis a the ray's coordinates at ta and tb bound X*_a (the ray is linear); every cell whose dilated
//      slab meets that range widened by s is visited (cell_low / cell_high: floor of the fp64 cell coordinate, stepped once
//      towards the neighbour whose margin holds the coordinate -- the floor is off by less than 2^-30 of a cell because
//      ops.mesh_face_grid keeps w above 2^-20 of the coordinate magnitude, and the margin EPS k w is below w / 2^12), so the
//      cell of the three k is visited: usually 1 or 2 cells per slab.
//   4. Every face of a visited cell is tested against the full [tmin, tmax]: a face met in several cells is tested again,
//      the minimum (t, face) is idempotent.
//   5. The walk stops before a slab whose entry parameter is strictly above best: entry parameters ascend in ray order (every
//      operation that makes them is monotone), so no later slab can hold a t* <= best.  An equal t* is still met: ties go to
//      the lower face index wherever it is listed.
// Every loop is bounded by the grid: <= 512 slabs x a cell rectangle inside the grid x a list length; an invalid ray leaves
// before the first loop; no input can make the kernel spin.  A plain 3D-DDA over nominal cells would NOT do: a ray running
// within the margin of a cell plane never enters the neighbour that may own the face.
//
// THE SLACK.  R = the largest magnitude among the components of o and of the mesh bounds, u = 2^-53, s = 2^-36 R = 2^17 u R.
// Inside the cut interval every coordinate of the ray is at most R + s in magnitude, so |t d_a| <= 2 R + s and every A = P - o
// at most 2 R.  (a) The traversal's own arithmetic: each computed plane parameter (p - o_a) / d_a and each computed coordinate
// o_a + t d_a is off by at most 8 u R in position (three roundings of quantities of magnitude <= 2 R + s), 2^-14 of s.  (b) The
// test: the transformed coordinates carry absolute errors <= 16 u R and are at most 4 R, so the edge functions are off by at
// most 2^8 u R^2; an accepted ray therefore passes, in exact arithmetic, within 2^9 u R kappa of the face, kappa = diameter^2 /
// (2 area) of the face's projection along the ray (1.15 for an equilateral triangle), and its computed t* is off by no more
// than that distance over |d|: X* is within 2^10 u R kappa of the face, which s / 4 = 2^15 u R covers for kappa up to 2^5.
// What the argument does NOT cover: a face with three distinct vertices on a line, or a sliver whose projected area is at the
// rounding level of its edge functions, can be "hit" by rounding noise at a parameter that has nothing to do with where the
// face is; brute force reports such a hit and the grid may not (the closest-point kernel has no such case).  Faces that repeat
// a vertex are never hit (above).
#include "bitgrid_device.h"

namespace mvip {
namespace raycast {

using namespace bitgrid;

static const int64_t INT_MAX64 = 2147483647;
constexpr int BLOCK = 256;
constexpr int MAX_DIRECTIONS = 255;
constexpr double EPS = 1.0 / 2097152.0;                      // 2^-21, the margin of csrc/mesh_distance.hip
constexpr double SLACK = 1.0 / 68719476736.0;                // 2^-36

struct Bounds {                                              // the fp32 bounds of the mesh's vertices
    float lx, ly, lz, hx, hy, hz;
};

struct Mesh {
    const float *__restrict__ verts;
    const int *__restrict__ faces;
    int V, F;
    Grid g;
    double wx, wy, wz;                                       // 1 / inv
    Bounds b;
    double rbox;                                             // the largest magnitude among the bounds
    const int *__restrict__ cell_offsets;
    const int *__restrict__ cell_faces;
};

struct Hit {
    double t, v, w;                                          // best t (+inf: none yet), V / det, W / det
    int face;
};

struct Axis {                                                // one axis of the ray and of the grid
    double o, d, og, w, lo, hi;
    int c, stride;
};

__host__ __device__ __forceinline__ double sel(int k, double x, double y, double z) { return k == 0 ? x : (k == 1 ? y : z); }
// (masks, not ?: -- the compiler turns a chain of selects between kernel arguments into a table in private memory)
__host__ __device__ __forceinline__ int sel(int k, int x, int y, int z) { return (x & -(int)(k == 0)) | (y & -(int)(k == 1)) | (z & -(int)(k == 2)); }
__host__ __device__ __forceinline__ Axis sel(int k, const Axis &x, const Axis &y, const Axis &z) {
    Axis r;
    r.o = sel(k, x.o, y.o, z.o);
    r.d = sel(k, x.d, y.d, z.d);
    r.og = sel(k, x.og, y.og, z.og);
    r.w = sel(k, x.w, y.w, z.w);
    r.lo = sel(k, x.lo, y.lo, z.lo);
    r.hi = sel(k, x.hi, y.hi, z.hi);
    r.c = sel(k, x.c, y.c, z.c);
    r.stride = sel(k, x.stride, y.stride, z.stride);
    return r;
}

__host__ __device__ __forceinline__ bool finite64(double x) { return fabs(x) <= 1.7976931348623157e308; }

// INVALID of the header, negated
__host__ __device__ __forceinline__ bool ray_valid(double ox, double oy, double oz, float dx, float dy, float dz, float tmin, float tmax) {
    return finite64(ox) && finite64(oy) && finite64(oz) && finite(dx) && finite(dy) && finite(dz) &&
           (dx != 0.f || dy != 0.f || dz != 0.f) && finite(tmin) && tmax >= tmin;      // NaN fails the comparison
}

__host__ __device__ __forceinline__ double plane_lo(const Axis &a, int k) { return a.og + (double)k * a.w * (1.0 + EPS); }
__host__ __device__ __forceinline__ double plane_hi(const Axis &a, int k) { return a.og + (double)k * a.w * (1.0 - EPS); }

// the clamped floor of the fp64 cell coordinate of x
__host__ __device__ __forceinline__ int cell_floor(const Axis &a, double x) {
    const double f = floor((x - a.og) / a.w);
    return f >= (double)a.c ? a.c - 1 : (f >= 0.0 ? (int)f : 0);
}
// the lowest cell whose dilated slab may hold x (x already lowered by the slack) / the highest (x already raised)
__host__ __device__ __forceinline__ int cell_low(const Axis &a, double x) {
    int j = cell_floor(a, x);
    if (j >= 1 && x <= plane_lo(a, j)) --j;
    return j;
}
__host__ __device__ __forceinline__ int cell_high(const Axis &a, double x) {
    int j = cell_floor(a, x);
    if (j + 1 <= a.c - 1 && x >= plane_hi(a, j + 1)) ++j;
    return j;
}

// step 1 of the traversal for one axis: false where the ray misses the bounds
__host__ __device__ __forceinline__ bool clip_axis(const Axis &a, double s, double &t0, double &t1) {
    if (a.d == 0.0) return a.o >= a.lo - s && a.o <= a.hi + s;
    const double p = ((a.lo - s) - a.o) / a.d, q = ((a.hi + s) - a.o) / a.d;
    t0 = fmax(t0, fmin(p, q));
    t1 = fmin(t1, fmax(p, q));
    return true;
}

// the cells j0 .. j1 of axis a that the ray can be in over [ta, tb] (step 3)
__host__ __device__ __forceinline__ void cell_range(const Axis &a, double s, double ta, double tb, int &j0, int &j1) {
    double x0 = a.o, x1 = a.o;
    if (a.d != 0.0) {
        x0 = a.o + ta * a.d;
        x1 = a.o + tb * a.d;
    }
    j0 = cell_low(a, fmin(x0, x1) - s);
    j1 = cell_high(a, fmax(x0, x1) + s);
}

// The valid ray (o, d, tmin, tmax) against the mesh: RESULT of the header in `hit` (ANY: the first accepted hit).  Callable on
// the host too (with host pointers in M), so that a CPU build can walk the very same code.
template <bool ANY, bool STATS>
__host__ __device__ __forceinline__ void trace(const Mesh &M, double ox, double oy, double oz, double dx, double dy, double dz, double tmin,
                                      double tmax, int skip, Hit &hit, unsigned &tests, unsigned &cells) {
    hit.t = __builtin_huge_val();
    hit.v = 0.0;
    hit.w = 0.0;
    hit.face = -1;
    // the shear of the ray
    const double mx = fabs(dx), my = fabs(dy), mz = fabs(dz);
    const int kz = (mx >= my && mx >= mz) ? 0 : (my >= mz ? 1 : 2);
    const bool neg = sel(kz, dx, dy, dz) < 0.0;
    const int k1 = kz == 2 ? 0 : kz + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    const int kx = neg ? k2 : k1, ky = neg ? k1 : k2;
    const double dkz = sel(kz, dx, dy, dz);
    const double Sx = sel(kx, dx, dy, dz) / dkz, Sy = sel(ky, dx, dy, dz) / dkz, Sz = 1.0 / dkz;
    // the axes, and the cut of step 1
    const Grid &g = M.g;
    const Axis X{ox, dx, (double)g.bx, M.wx, (double)M.b.lx, (double)M.b.hx, g.cx, g.cy * g.cz};
    const Axis Y{oy, dy, (double)g.by, M.wy, (double)M.b.ly, (double)M.b.hy, g.cy, g.cz};
    const Axis Z{oz, dz, (double)g.bz, M.wz, (double)M.b.lz, (double)M.b.hz, g.cz, 1};
    const double s = SLACK * fmax(fmax(fabs(ox), fabs(oy)), fmax(fabs(oz), M.rbox));
    double t0 = tmin, t1 = tmax;
    if (!clip_axis(X, s, t0, t1) || !clip_axis(Y, s, t0, t1) || !clip_axis(Z, s, t0, t1) || !(t0 <= t1)) return;
    // step 2
    const double px = mx * (double)g.ix, py = my * (double)g.iy, pz = mz * (double)g.iz;
    const int m = (px >= py && px >= pz) ? 0 : (py >= pz ? 1 : 2);
    const int ia = m == 2 ? 0 : m + 1, ib = ia == 2 ? 0 : ia + 1;
    const Axis Am = sel(m, X, Y, Z), Aa = sel(ia, X, Y, Z), Ab = sel(ib, X, Y, Z);
    const bool up = Am.d > 0.0;
    int ka, kb;
    cell_range(Am, s, t0, t1, ka, kb);
    bool done = false;
    for (int step = 0; step <= kb - ka && !done; ++step) {
        const int k = up ? ka + step : kb - step;
        const double below = k == 0 ? -__builtin_huge_val() : plane_hi(Am, k) - s;
        const double above = k == Am.c - 1 ? __builtin_huge_val() : plane_lo(Am, k + 1) + s;
        const double t_in = ((up ? below : above) - Am.o) / Am.d, t_out = ((up ? above : below) - Am.o) / Am.d;
        if (hit.t < t_in) break;                                          // step 5
        const double ta = fmax(t0, t_in), tb = fmin(fmin(t1, hit.t), t_out);
        if (!(ta <= tb)) continue;
        int a0, a1, b0, b1;
        cell_range(Aa, s, ta, tb, a0, a1);
        cell_range(Ab, s, ta, tb, b0, b1);
        for (int ja = a0; ja <= a1 && !done; ++ja) {
            for (int jb = b0; jb <= b1 && !done; ++jb) {
                const int l = k * Am.stride + ja * Aa.stride + jb * Ab.stride;
                if (STATS) ++cells;
                const int end = M.cell_offsets[l + 1];
                for (int i = M.cell_offsets[l]; i < end; ++i) {
                    const int f = M.cell_faces[i];
                    if ((unsigned)f >= (unsigned)M.F || f == skip) continue;      // (the first never: the grid is of this mesh)
                    const int a = M.faces[3 * f], b = M.faces[3 * f + 1], c = M.faces[3 * f + 2];
                    if ((unsigned)a >= (unsigned)M.V || (unsigned)b >= (unsigned)M.V || (unsigned)c >= (unsigned)M.V) continue;
                    if (STATS) ++tests;
                    // RAY - TRIANGLE of the header
                    double e0 = (double)M.verts[3 * a] - ox, e1 = (double)M.verts[3 * a + 1] - oy, e2 = (double)M.verts[3 * a + 2] - oz;
                    double Az = sel(kz, e0, e1, e2);
                    const double Ax = sel(kx, e0, e1, e2) - Sx * Az, Ay = sel(ky, e0, e1, e2) - Sy * Az;
                    Az = Sz * Az;
                    e0 = (double)M.verts[3 * b] - ox, e1 = (double)M.verts[3 * b + 1] - oy, e2 = (double)M.verts[3 * b + 2] - oz;
                    double Bz = sel(kz, e0, e1, e2);
                    const double Bx = sel(kx, e0, e1, e2) - Sx * Bz, By = sel(ky, e0, e1, e2) - Sy * Bz;
                    Bz = Sz * Bz;
                    e0 = (double)M.verts[3 * c] - ox, e1 = (double)M.verts[3 * c + 1] - oy, e2 = (double)M.verts[3 * c + 2] - oz;
                    double Cz = sel(kz, e0, e1, e2);
                    const double Cx = sel(kx, e0, e1, e2) - Sx * Cz, Cy = sel(ky, e0, e1, e2) - Sy * Cz;
                    Cz = Sz * Cz;
                    const double U = Cx * By - Cy * Bx, Vv = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
                    if (!((U >= 0.0 && Vv >= 0.0 && W >= 0.0) || (U <= 0.0 && Vv <= 0.0 && W <= 0.0))) continue;
                    const double det = (U + Vv) + W;
                    if (det == 0.0) continue;
                    const double t = ((U * Az + Vv * Bz) + W * Cz) / det;
                    if (!(t >= tmin && t <= tmax)) continue;
                    if (t < hit.t || (t == hit.t && f < hit.face)) {
                        hit.t = t;
                        hit.v = Vv / det;
                        hit.w = W / det;
                        hit.face = f;
                        if (ANY) {
                            done = true;
                            break;
                        }
                    }
                }
            }
        }
    }
}

// stats: [0] the ray-face tests, [1] 64 x the tests of each wave's busiest lane, [2] the cells visited -- integer atomics, once
// per wave
__device__ __forceinline__ void add_stats(unsigned long long *stats, unsigned tests, unsigned cells) {
    unsigned long long t = tests, c = cells;
    unsigned m = tests;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        t += __shfl_xor(t, o, 64);
        c += __shfl_xor(c, o, 64);
        m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && (t || c)) {
        atomicAdd(stats, t);
        atomicAdd(stats + 1, 64ull * m);
        atomicAdd(stats + 2, c);
    }
}

__global__ __launch_bounds__(BLOCK) void clear_stats_kernel(unsigned long long *stats) {
    if (threadIdx.x < 3 && blockIdx.x == 0) stats[threadIdx.x] = 0ull;
}

template <bool ANY, bool STATS>
__global__ __launch_bounds__(BLOCK) void cast_kernel(const float *__restrict__ origins, const float *__restrict__ dirs,
                                                    const float *__restrict__ tmins, const float *__restrict__ tmaxs, float tmin0,
                                                    float tmax0, const int *__restrict__ skips, int N, Mesh M,
                                                    int *__restrict__ out_face, float *__restrict__ out_t,
                                                    float *__restrict__ out_bary, unsigned long long *stats) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    unsigned tests = 0, cells = 0;
    if (n < N) {
        const float ox = origins[3 * n], oy = origins[3 * n + 1], oz = origins[3 * n + 2];
        const float dx = dirs[3 * n], dy = dirs[3 * n + 1], dz = dirs[3 * n + 2];
        const float tmin = tmins ? tmins[n] : tmin0, tmax = tmaxs ? tmaxs[n] : tmax0;
        const float nan = __builtin_nanf("");
        int face = -1;
        float t = nan, bv = nan, bw = nan;
        if (ray_valid((double)ox, (double)oy, (double)oz, dx, dy, dz, tmin, tmax)) {
            Hit hit;
            trace<ANY, STATS>(M, (double)ox, (double)oy, (double)oz, (double)dx, (double)dy, (double)dz, (double)tmin, (double)tmax,
                              skips ? skips[n] : -1, hit, tests, cells);
            face = hit.face;
            t = (float)hit.t;                                              // +inf for a miss
            if (face >= 0) {
                bv = (float)hit.v;
                bw = (float)hit.w;
            }
        }
        out_face[n] = face;
        if (out_t) out_t[n] = t;
        if (out_bary) {
            out_bary[2 * n] = bv;
            out_bary[2 * n + 1] = bw;
        }
    }
    if (STATS) add_stats(stats, tests, cells);
}

// FACE OPENNESS of the header, one thread per face
template <bool STATS>
__global__ __launch_bounds__(BLOCK) void openness_kernel(Mesh M, const float *__restrict__ directions, int K, float max_dist,
                                                        int *__restrict__ counts, unsigned long long *stats) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    unsigned tests = 0, cells = 0;
    if (f < M.F) {
        int fo = 0, ft = 0, bo = 0, bt = 0;
        const int a = M.faces[3 * f], b = M.faces[3 * f + 1], c = M.faces[3 * f + 2];
        if ((unsigned)a < (unsigned)M.V && (unsigned)b < (unsigned)M.V && (unsigned)c < (unsigned)M.V) {
            const double ax = (double)M.verts[3 * a], ay = (double)M.verts[3 * a + 1], az = (double)M.verts[3 * a + 2];
            const double bx = (double)M.verts[3 * b], by = (double)M.verts[3 * b + 1], bz = (double)M.verts[3 * b + 2];
            const double cx = (double)M.verts[3 * c], cy = (double)M.verts[3 * c + 1], cz = (double)M.verts[3 * c + 2];
            const double ox = ((ax + bx) + cx) / 3.0, oy = ((ay + by) + cy) / 3.0, oz = ((az + bz) + cz) / 3.0;
            const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
            const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            for (int k = 0; k < K; ++k) {
                const float dx = directions[3 * k], dy = directions[3 * k + 1], dz = directions[3 * k + 2];
                const double nd = (nx * (double)dx + ny * (double)dy) + nz * (double)dz;
                if (!(nd > 0.0 || nd < 0.0)) continue;
                bool open = false;
                if (ray_valid(ox, oy, oz, dx, dy, dz, 0.f, max_dist)) {
                    Hit hit;
                    trace<true, STATS>(M, ox, oy, oz, (double)dx, (double)dy, (double)dz, 0.0, (double)max_dist, f, hit, tests, cells);
                    open = hit.face < 0;
                }
                if (nd > 0.0) {
                    ++ft;
                    fo += open;
                } else {
                    ++bt;
                    bo += open;
                }
            }
        }
        counts[f] = fo;
        counts[M.F + f] = ft;
        counts[2 * M.F + f] = bo;
        counts[3 * M.F + f] = bt;
    }
    if (STATS) add_stats(stats, tests, cells);
}

static inline bool count_ok(int64_t n) { return n >= 0 && n <= INT_MAX64; }

// the checks every entry point makes of its mesh and grid arguments; fills M
static inline bool mesh_from_args(const float *verts, const int *faces, int64_t V, int64_t F, const float *box, const int *cells,
                                  const float *bounds, const int *cell_offsets, const int *cell_faces, int64_t n_pairs, Mesh &M) {
    static const int some_words = 0;
    if (!(V >= 1 && V <= INT_MAX64 && F >= 1 && 3 * F <= INT_MAX64) || !count_ok(n_pairs)) return false;
    if (!grid_from_args(box, cells, &some_words, M.g) || !bounds) return false;
    if (!verts || !faces || !cell_offsets || (n_pairs > 0 && !cell_faces)) return false;
    double r = 0.0;
    for (int a = 0; a < 6; ++a) {
        if (!finite(bounds[a])) return false;
        r = fmax(r, fabs((double)bounds[a]));
    }
    for (int a = 0; a < 3; ++a)
        if (!(bounds[a] <= bounds[3 + a])) return false;
    M.verts = verts;
    M.faces = faces;
    M.V = (int)V;
    M.F = (int)F;
    M.wx = 1.0 / (double)M.g.ix;
    M.wy = 1.0 / (double)M.g.iy;
    M.wz = 1.0 / (double)M.g.iz;
    M.b = Bounds{bounds[0], bounds[1], bounds[2], bounds[3], bounds[4], bounds[5]};
    M.rbox = r;
    M.cell_offsets = cell_offsets;
    M.cell_faces = cell_faces;
    return true;
}

}  // namespace raycast
}  // namespace mvip

using namespace mvip;
namespace rc = mvip::raycast;

extern "C" int mvip_mesh_raycast(const float *origins, const float *dirs, const float *tmin, const float *tmax, float tmin_all,
                                 float tmax_all, const int *skip, int64_t n_rays, const float *verts, const int *faces,
                                 int64_t n_verts, int64_t n_faces, const float *box, const int *cells, const float *bounds,
                                 const int *cell_offsets, const int *cell_faces, int64_t n_pairs, int any_hit, int *face, float *t,
                                 float *bary, void *stats, void *stream) {
    rc::Mesh M;
    if (!rc::mesh_from_args(verts, faces, n_verts, n_faces, box, cells, bounds, cell_offsets, cell_faces, n_pairs, M)) return MVIP_EINVAL;
    if (!rc::count_ok(n_rays) || 3 * n_rays > rc::INT_MAX64 || (any_hit != 0 && any_hit != 1)) return MVIP_EINVAL;
    if (n_rays > 0 && (!origins || !dirs || !face)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    unsigned long long *st = (unsigned long long *)stats;
    if (st) hipLaunchKernelGGL(rc::clear_stats_kernel, dim3(1), dim3(rc::BLOCK), 0, s, st);
    if (n_rays > 0) {
        const dim3 grid(blocks_for(n_rays, rc::BLOCK)), block(rc::BLOCK);
        const int N = (int)n_rays;
        if (any_hit && st)
            hipLaunchKernelGGL((rc::cast_kernel<true, true>), grid, block, 0, s, origins, dirs, tmin, tmax, tmin_all, tmax_all, skip, N, M,
                               face, t, bary, st);
        else if (any_hit)
            hipLaunchKernelGGL((rc::cast_kernel<true, false>), grid, block, 0, s, origins, dirs, tmin, tmax, tmin_all, tmax_all, skip, N,
                               M, face, t, bary, st);
        else if (st)
            hipLaunchKernelGGL((rc::cast_kernel<false, true>), grid, block, 0, s, origins, dirs, tmin, tmax, tmin_all, tmax_all, skip, N,
                               M, face, t, bary, st);
        else
            hipLaunchKernelGGL((rc::cast_kernel<false, false>), grid, block, 0, s, origins, dirs, tmin, tmax, tmin_all, tmax_all, skip, N,
                               M, face, t, bary, st);
    }
    return check_launch();
}

extern "C" int mvip_mesh_face_openness(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const float *box,
                                       const int *cells, const float *bounds, const int *cell_offsets, const int *cell_faces,
                                       int64_t n_pairs, const float *directions, int n_dirs, float max_dist, int *counts,
                                       void *stats, void *stream) {
    rc::Mesh M;
    if (!rc::mesh_from_args(verts, faces, n_verts, n_faces, box, cells, bounds, cell_offsets, cell_faces, n_pairs, M)) return MVIP_EINVAL;
    if (n_dirs < 0 || n_dirs > rc::MAX_DIRECTIONS || 4 * n_faces > rc::INT_MAX64 || !(max_dist >= 0.f) || !counts) return MVIP_EINVAL;
    if (n_dirs > 0 && !directions) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    unsigned long long *st = (unsigned long long *)stats;
    if (st) hipLaunchKernelGGL(rc::clear_stats_kernel, dim3(1), dim3(rc::BLOCK), 0, s, st);
    const dim3 grid(blocks_for(n_faces, rc::BLOCK)), block(rc::BLOCK);
    if (st)
        hipLaunchKernelGGL(rc::openness_kernel<true>, grid, block, 0, s, M, directions, n_dirs, max_dist, counts, st);
    else
        hipLaunchKernelGGL(rc::openness_kernel<false>, grid, block, 0, s, M, directions, n_dirs, max_dist, counts, st);
    return check_launch();
}
