// Signed mesh distance (beyond the reference, which has no mesh export at all): the closest point of csrc/mesh_distance.hip with a
// sign from the angle-weighted pseudonormal of the closest feature (Baerentzen and Aanaes, "Signed distance computation using
// the angle weighted pseudonormal", 2005), for N query points or for the points of a lattice that the kernel generates
// (ops.mesh_vertex_pseudonormals / mesh_signed_distance / mesh_signed_distance_lattice, mesh.signed_distance / sdf_grid /
// remesh).  THE statement of the definitions; restated for the tests in tests/mesh_sdf_numpy.py.
//
// All arithmetic is fp64 on the widened fp32 inputs, every expression associates as written (x . y = (x0 y0 + x1 y1) + x2 y2,
// the library is built with -ffp-contract=off), results are rounded to fp32 once.
//
// CLOSEST FEATURE.  face(p), q and d2 are exactly those of csrc/mesh_distance.hip: the same candidates in the same order, strict
// replacement, the lowest face index among equals.  In addition the candidate of the winning face that supplied q is recorded
// (csrc/mesh_distance_device.h): 0 the interior; segment k (0: ab, 1: bc, 2: ca) with 0 < t < 1: 1 + k, an edge; with t == 0
// (ee == 0 included): 4 + k; with t == 1: 4 + (k + 1) % 3 -- a vertex of the face, 4 + its position in the face.
//
// PSEUDONORMAL n.  N(f) = (b - a) x (c - a);  U(f) = N / sqrt(N . N) per component, (0, 0, 0) if N . N == 0.
//   interior: n = N(f).
//   edge h = 3 f + k: n = U(f) + U(twin[h] / 3) per component if twin[h] >= 0, else U(f); twin is that of ops.mesh_edge_table
//     (exactly two half-edges on the edge), so the sum is the same whichever of the two faces won.
//   vertex v: n = P[v] = the sum over the corners c = 3 f + k of v, in corner-table order, of theta_c U(f) per component,
//     theta_c = atan2(sqrt(X . X), u . w), X = u x w, u = faces[f, (k + 1) % 3] - v, w = faces[f, (k + 2) % 3] - v (the two
//     edges that leave the corner).  P is [V, 3] fp64, unnormalised, (0, 0, 0) for a vertex without a corner.
//
// SIGN.  s = n . (p - q) with q unrounded; sdist = fp32(sqrt(d2)), negated iff s < 0 and d2 > 0.  On a closed, consistently
// oriented manifold mesh negative means inside; on anything else the value is still defined by the above.  Nothing is refused.
//
// BAND.  max_dist = B (+inf: none).  A query is out of band iff its d2 > B B; it then gets face -1, feature -1 and NaN for
// sdist and point, as a query with a NaN or infinite coordinate does.  The walk stops once min(best, B B) (1 + 2^-40) < L L
// (csrc/mesh_distance_device.h): no face within the band is lost, so in-band membership and values depend neither on the grid
// nor on B.
//
// LATTICE MODE.  Instead of points the kernel takes lo[3], h[3] (fp32) and counts[3]: query n = (i * ny + j) * nz + k is the
// point fp32(fp32(i) h) + lo per axis -- mesh.grid_axes' expression.  No [N, 3] tensor of points exists.
//
// atan2 is the one operation here that is not reproducible across libraries: P is pinned to the restatement within a bound,
// and the signed distance bit for bit given P.
#include "mesh_distance_device.h"

namespace mvip {
namespace meshsdf {

using namespace bitgrid;
using namespace meshdist;

static const int64_t INT_MAX64 = 2147483647;
constexpr int BLOCK = 256;

struct Lattice {
    float lx, ly, lz, hx, hy, hz;
    int nx, ny, nz;                                           // nx == 0: points mode
};

// U(f) of the header; zeros for an index outside [0, V).  N(f) comes with it.
__host__ __device__ __forceinline__ void face_normals(const float *__restrict__ verts, const int *__restrict__ faces, int V, int f,
                                                      double &nx, double &ny, double &nz, double &ux, double &uy, double &uz) {
    nx = ny = nz = ux = uy = uz = 0.0;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return;
    const double ax = (double)verts[3 * a], ay = (double)verts[3 * a + 1], az = (double)verts[3 * a + 2];
    cross3((double)verts[3 * b] - ax, (double)verts[3 * b + 1] - ay, (double)verts[3 * b + 2] - az, (double)verts[3 * c] - ax,
           (double)verts[3 * c + 1] - ay, (double)verts[3 * c + 2] - az, nx, ny, nz);
    const double nn = dot3(nx, ny, nz, nx, ny, nz);
    if (nn > 0.0) {
        const double len = sqrt(nn);
        ux = nx / len;
        uy = ny / len;
        uz = nz / len;
    }
}

// theta_c of the header for corner k of face f (its indices in range)
__host__ __device__ __forceinline__ double corner_angle(const float *__restrict__ verts, const int *__restrict__ faces, int f, int k) {
    const int v = faces[3 * f + k], b = faces[3 * f + (k == 2 ? 0 : k + 1)], c = faces[3 * f + (k == 0 ? 2 : k - 1)];
    const double vx = (double)verts[3 * v], vy = (double)verts[3 * v + 1], vz = (double)verts[3 * v + 2];
    const double ux = (double)verts[3 * b] - vx, uy = (double)verts[3 * b + 1] - vy, uz = (double)verts[3 * b + 2] - vz;
    const double wx = (double)verts[3 * c] - vx, wy = (double)verts[3 * c + 1] - vy, wz = (double)verts[3 * c + 2] - vz;
    double xx, xy, xz;
    cross3(ux, uy, uz, wx, wy, wz, xx, xy, xz);
    return atan2(sqrt(dot3(xx, xy, xz, xx, xy, xz)), dot3(ux, uy, uz, wx, wy, wz));
}

// P[v] of the header from the corner list corners[lo:hi]
__host__ __device__ __forceinline__ void vertex_pseudonormal(const float *__restrict__ verts, const int *__restrict__ faces, int V,
                                                             int F, const int *__restrict__ corners, int lo, int hi, double &px,
                                                             double &py, double &pz) {
    px = py = pz = 0.0;
    for (int u = lo; u < hi; ++u) {
        const int c = corners[u];
        if ((unsigned)c >= 3u * (unsigned)F) continue;            // never: the table is of these faces
        const int f = c / 3, k = c - 3 * f;
        const int a = faces[3 * f], b = faces[3 * f + 1], cc = faces[3 * f + 2];
        if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)cc >= (unsigned)V) continue;
        double nx, ny, nz, ux, uy, uz;
        face_normals(verts, faces, V, f, nx, ny, nz, ux, uy, uz);
        const double theta = corner_angle(verts, faces, f, k);
        px = px + theta * ux;
        py = py + theta * uy;
        pz = pz + theta * uz;
    }
}

// SIGN of the header for the winning face f of p, its feature and its unrounded q: true iff s < 0
__host__ __device__ __forceinline__ bool sign_negative(const float *__restrict__ verts, const int *__restrict__ faces, int V, int F,
                                                       const int *__restrict__ twin, const double *__restrict__ P, int f, int feat,
                                                       double px, double py, double pz, double qx, double qy, double qz) {
    double nx, ny, nz, ux, uy, uz;
    face_normals(verts, faces, V, f, nx, ny, nz, ux, uy, uz);
    if (feat >= 4) {
        const int v = faces[3 * f + (feat - 4)];
        nx = P[3 * (size_t)v];
        ny = P[3 * (size_t)v + 1];
        nz = P[3 * (size_t)v + 2];
    } else if (feat >= 1) {
        const int t = twin[3 * f + (feat - 1)];
        nx = ux;
        ny = uy;
        nz = uz;
        if (t >= 0 && t < 3 * F) {
            double mx, my, mz, wx, wy, wz;
            face_normals(verts, faces, V, t / 3, mx, my, mz, wx, wy, wz);
            nx = ux + wx;
            ny = uy + wy;
            nz = uz + wz;
        }
    }
    return dot3(nx, ny, nz, px - qx, py - qy, pz - qz) < 0.0;
}

__global__ __launch_bounds__(BLOCK) void vertex_pseudonormal_kernel(const float *__restrict__ verts, const int *__restrict__ faces,
                                                                   int V, int F, const int *__restrict__ offsets,
                                                                   const int *__restrict__ corners, double *__restrict__ P) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    double px, py, pz;
    vertex_pseudonormal(verts, faces, V, F, corners, offsets[v], offsets[v + 1], px, py, pz);
    P[3 * (size_t)v] = px;
    P[3 * (size_t)v + 1] = py;
    P[3 * (size_t)v + 2] = pz;
}

template <bool STATS>
__global__ __launch_bounds__(BLOCK) void signed_query_kernel(const float *__restrict__ points, Lattice lat, int N,
                                                            const float *__restrict__ verts, const int *__restrict__ faces, int V,
                                                            int F, Grid g, double wx, double wy, double wz,
                                                            const int *__restrict__ cell_offsets, const int *__restrict__ cell_faces,
                                                            const int *__restrict__ twin, const double *__restrict__ P, double cap2,
                                                            float *__restrict__ out_sdist, int *__restrict__ out_face,
                                                            float *__restrict__ out_point, int *__restrict__ out_feature,
                                                            unsigned long long *stats) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    if (!STATS && n >= N) return;                              // (the counting variant keeps whole waves for its shuffles)
    float fx = __builtin_nanf(""), fy = fx, fz = fx;
    if (n >= N) {
    } else if (lat.nx > 0) {
        const int k = n % lat.nz, ij = n / lat.nz, j = ij % lat.ny, i = ij / lat.ny;
        fx = (float)i * lat.hx + lat.lx;
        fy = (float)j * lat.hy + lat.ly;
        fz = (float)k * lat.hz + lat.lz;
    } else {
        fx = points[3 * (size_t)n];
        fy = points[3 * (size_t)n + 1];
        fz = points[3 * (size_t)n + 2];
    }
    unsigned tests = 0;
    double best = __builtin_huge_val(), bqx = 0.0, bqy = 0.0, bqz = 0.0;
    int bf = -1;
    if (finite(fx) && finite(fy) && finite(fz))
        shell_walk<STATS>(fx, fy, fz, verts, faces, V, F, g, wx, wy, wz, cell_offsets, cell_faces, cap2, best, bf, bqx, bqy, bqz,
                          tests);
    const float nan = __builtin_nanf("");
    float sd = nan, qx = nan, qy = nan, qz = nan;
    int feat = -1;
    if (bf >= 0 && !(best > cap2)) {
        const double px = (double)fx, py = (double)fy, pz = (double)fz;
        double d2, rx, ry, rz;
        point_face(verts, faces, V, bf, px, py, pz, d2, rx, ry, rz, feat);             // the winning face again: d2 == best, r == bq
        sd = (float)sqrt(d2);
        if (d2 > 0.0 && sign_negative(verts, faces, V, F, twin, P, bf, feat, px, py, pz, rx, ry, rz)) sd = -sd;
        qx = (float)rx;
        qy = (float)ry;
        qz = (float)rz;
    } else {
        bf = -1;
    }
    if (n < N) {
        out_sdist[n] = sd;
        out_face[n] = bf;
        if (out_point) {
            out_point[3 * (size_t)n] = qx;
            out_point[3 * (size_t)n + 1] = qy;
            out_point[3 * (size_t)n + 2] = qz;
        }
        if (out_feature) out_feature[n] = feat;
    }
    if (STATS) {                                              // as query_kernel<true> of csrc/mesh_distance.hip
        unsigned long long t = tests;
        unsigned m = tests;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            t += __shfl_xor(t, o, 64);
            m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
        }
        if ((threadIdx.x & 63) == 0 && t) {
            atomicAdd(stats, t);
            atomicAdd(stats + 1, 64ull * m);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void clear_stats_kernel(unsigned long long *stats) {
    if (threadIdx.x < 2 && blockIdx.x == 0) stats[threadIdx.x] = 0ull;
}

}  // namespace meshsdf
}  // namespace mvip

#ifndef MVIP_MESH_SDF_NO_ENTRY_POINTS
using namespace mvip;
namespace ms = mvip::meshsdf;

extern "C" int mvip_mesh_vertex_pseudonormals(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces,
                                              const int *offsets, const int *corners, double *pseudonormals, void *stream) {
    if (n_verts < 0 || n_verts > ms::INT_MAX64 || n_faces < 0 || 3 * n_faces > ms::INT_MAX64) return MVIP_EINVAL;
    if (n_verts > 0 && (!verts || !offsets || !pseudonormals)) return MVIP_EINVAL;
    if (n_faces > 0 && (!faces || !corners)) return MVIP_EINVAL;
    if (n_verts > 0)
        hipLaunchKernelGGL(ms::vertex_pseudonormal_kernel, dim3(blocks_for(n_verts, ms::BLOCK)), dim3(ms::BLOCK), 0, as_stream(stream),
                           verts, faces, (int)n_verts, (int)n_faces, offsets, corners, pseudonormals);
    return check_launch();
}

extern "C" int mvip_mesh_signed_distance(const float *points, const float *lattice_lo, const float *lattice_h,
                                         const int *lattice_counts, int64_t n_points, const float *verts, const int *faces,
                                         int64_t n_verts, int64_t n_faces, const float *box, const int *cells,
                                         const int *cell_offsets, const int *cell_faces, int64_t n_pairs, const int *twin,
                                         const double *pseudonormals, double max_dist, float *sdist, int *face, float *point,
                                         int *feature, void *stats, void *stream) {
    bitgrid::Grid g;
    static const int some_words = 0;
    if (n_verts < 1 || n_verts > ms::INT_MAX64 || n_faces < 1 || 3 * n_faces > ms::INT_MAX64) return MVIP_EINVAL;
    if (!bitgrid::grid_from_args(box, cells, &some_words, g)) return MVIP_EINVAL;
    if (n_pairs < 0 || n_pairs > ms::INT_MAX64 || n_points < 0 || n_points > ms::INT_MAX64) return MVIP_EINVAL;
    if (!(max_dist >= 0.0)) return MVIP_EINVAL;                                        // NaN fails too
    if (!verts || !faces || !cell_offsets || (n_pairs > 0 && !cell_faces) || !twin || !pseudonormals) return MVIP_EINVAL;
    ms::Lattice lat{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0, 0};
    const bool lattice = lattice_lo || lattice_h || lattice_counts;
    if (lattice) {
        if (points || !lattice_lo || !lattice_h || !lattice_counts) return MVIP_EINVAL;
        for (int a = 0; a < 3; ++a)
            if (lattice_counts[a] < 1 || !finite(lattice_lo[a]) || !finite(lattice_h[a]) || !(lattice_h[a] > 0.f)) return MVIP_EINVAL;
        if ((int64_t)lattice_counts[0] * lattice_counts[1] > ms::INT_MAX64 ||
            (int64_t)lattice_counts[0] * lattice_counts[1] * lattice_counts[2] != n_points)
            return MVIP_EINVAL;
        lat = ms::Lattice{lattice_lo[0], lattice_lo[1], lattice_lo[2], lattice_h[0], lattice_h[1], lattice_h[2],
                          lattice_counts[0], lattice_counts[1], lattice_counts[2]};
    } else if (n_points > 0 && !points) {
        return MVIP_EINVAL;
    }
    if (n_points > 0 && (!sdist || !face)) return MVIP_EINVAL;
    if (point && 3 * n_points > ms::INT_MAX64) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    if (stats) hipLaunchKernelGGL(ms::clear_stats_kernel, dim3(1), dim3(ms::BLOCK), 0, s, (unsigned long long *)stats);
    if (n_points > 0) {
        const double wx = 1.0 / (double)g.ix, wy = 1.0 / (double)g.iy, wz = 1.0 / (double)g.iz;
        const dim3 grid(blocks_for(n_points, ms::BLOCK)), block(ms::BLOCK);
        if (stats)
            hipLaunchKernelGGL(ms::signed_query_kernel<true>, grid, block, 0, s, points, lat, (int)n_points, verts, faces, (int)n_verts,
                               (int)n_faces, g, wx, wy, wz, cell_offsets, cell_faces, twin, pseudonormals, max_dist * max_dist, sdist,
                               face, point, feature, (unsigned long long *)stats);
        else
            hipLaunchKernelGGL(ms::signed_query_kernel<false>, grid, block, 0, s, points, lat, (int)n_points, verts, faces, (int)n_verts,
                               (int)n_faces, g, wx, wy, wz, cell_offsets, cell_faces, twin, pseudonormals, max_dist * max_dist, sdist,
                               face, point, feature, (unsigned long long *)nullptr);
    }
    return check_launch();
}
#endif
