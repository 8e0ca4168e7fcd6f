// Mesh-to-mesh distance (beyond the reference, which has no mesh export at all): the closest point of an indexed triangle mesh
// to each of N query points, found on a uniform grid of face lists, and deterministic surface samples (ops.mesh_face_grid /
// mesh_closest_point / mesh_sample_faces, evaluate.mesh_distance_metrics).  THE statement of the definitions; restated for
// the tests in tests/mesh_distance_numpy.py.
//
// verts [V, 3] fp32, faces [F, 3] int32, points [N, 3] fp32.  All arithmetic is fp64 on the widened fp32 inputs, every
// expression associates as written (x . y = (x0 y0 + x1 y1) + x2 y2, the library is built with -ffp-contract=off), results are
// rounded to fp32 once.
//
// POINT - TRIANGLE.  For a point p and a face (a, b, c) the squared distance d2 and the closest point q are the first of four
// candidates, in this order, a later one replacing an earlier one only where its d2 is STRICTLY smaller:
//   interior: N = (b - a) x (c - a), nn = N . N.  Taken iff nn > 0 and N . ((b - a) x (p - a)) >= 0 and
//     N . ((c - b) x (p - b)) >= 0 and N . ((a - c) x (p - c)) >= 0.  s = N . (p - a), d2 = s s / nn, q = p - N (s / nn).
//   segments ab, bc, ca: for the segment from u along e (e = b - a from a, c - b from b, a - c from c): ee = e . e,
//     t = ((p - u) . e) / ee set to 0 where t < 0 and to 1 where t > 1, t = 0 where ee == 0; q = u + t e, d2 = (p - q) . (p - q).
// A zero-area face is its segments, a point face its point; nothing divides by zero.
//
// CLOSEST POINT ON A MESH.  face(p) = the face of smallest d2, the lowest face index among equals; point = fp32(q) of that
// face, dist = fp32(sqrt(d2)).  A query with a NaN or infinite coordinate: face -1, point and dist NaN.  THE RESULT DOES NOT
// DEPEND ON THE GRID below; the grid only decides which faces are tested.
//
// THE FACE GRID.  The box conventions of csrc/bitgrid_device.h: origin o, inv (fp32, per axis), (cx, cy, cz) cells, each
// 1..512.  g(x) = floorf((x - o) * inv) in fp32 is the cell coordinate of a coordinate x: a MONOTONE function of x (an fp32
// subtraction of a constant, a multiplication by a positive constant and floorf all are).  A face is entered in every cell
// of the product, over the axes, of [clamp(g(min)), clamp(g(max))], min / max its smallest / largest fp32 vertex coordinate
// and clamp to 0 .. c - 1.  Lists: per-face pair counts -> exclusive 64-bit scan (compact::scan_kernel) -> one thread per pair
// finds its face by bisection and writes (cell, face), so the pairs are in face order -> the lists of csrc/mesh_ops.hip over
// the cell keys (mvip_mesh_corner_table), which are ascending in the pair and so in the face -> the pairs' faces gathered.
//
// THE MARGIN.  With w = 1 / inv (fp64) and EPS = 2^-21, the plane below cell k is at lo(k) = o + k w (1 + EPS), the plane above
// cell k - 1 at hi(k) = o + k w (1 - EPS).  If g(x) < k for an integer k >= 1 then x < o + k w (1 + 2^-22): were x - o >=
// k w (1 + 2^-22), the two fp32 roundings (each a factor >= 1 - 2^-24) would leave a product >= k, and g(x) >= k.  Likewise
// g(x) >= k implies x - o >= k w (1 - 2^-22).  So a face whose cell range ends below k lies wholly below lo(k), one whose range
// starts at k or above wholly above hi(k): every face's box is in effect DILATED by 2^-21 of its distance from the origin plane,
// of which 2^-22 covers the fp32 cell assignment and the other 2^-22 (k w 2^-22 >= w 2^-22 in absolute terms) the fp64 rounding
// of q and s (a few 2^-53 of the coordinate magnitude; ops.mesh_face_grid keeps w above 2^-20 of that magnitude).
//
// THE QUERY, one thread per point.  (ci, cj, ck) = the clamped cell of p.  Shells of Chebyshev radius r = 0, 1, 2, ... around
// it: the cells of the block [ci - r, ci + r] x ... (cut to the grid) that are not in the block of r - 1.  After shell r a face
// not yet met is in no cell of the block, so on some axis its cell range misses [c - r, c + r]: it lies wholly beyond lo(c - r)
// (if c - r >= 1) or hi(c + r + 1) (if c + r + 1 <= cells - 1) of that axis; the sides on the grid boundary have nothing beyond
// them.  L = the minimum over those interior sides of max(0, signed distance from p to the plane) is a lower bound on the
// distance of every face not yet met, wherever p lies (the clamped cell need not contain p: the bound never uses that it
// does).  Stop when best (1 + 2^-40) < L L, strictly -- no unmet face can tie -- or when the block covers the grid.  A face met in
// several cells is tested again: the minimum is idempotent.
//
// POINT - TRIANGLE and THE QUERY's walk are written in csrc/mesh_distance_device.h, which csrc/mesh_sdf.hip shares.
#include "compact_device.h"
#include "mesh_distance_device.h"

namespace mvip {
namespace meshdist {

using namespace bitgrid;
using namespace compact;

static const int64_t INT_MAX64 = 2147483647;
constexpr int MAX_SUBDIVISION = 1024;

struct Range {
    int i0, i1, j0, j1, k0, k1;
};

// the cell ranges of face f; false (and the flag bits) for an index outside [0, V) or a vertex that is not finite
__device__ __forceinline__ bool face_range(const float *__restrict__ verts, const int *__restrict__ faces, int V, const Grid &g,
                                           int f, Range &r, int *flag) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) {
        if (flag) atomicOr(flag, 1);
        return false;
    }
    const float ax = verts[3 * a], ay = verts[3 * a + 1], az = verts[3 * a + 2];
    const float bx = verts[3 * b], by = verts[3 * b + 1], bz = verts[3 * b + 2];
    const float cx = verts[3 * c], cy = verts[3 * c + 1], cz = verts[3 * c + 2];
    if (!(finite(ax) && finite(ay) && finite(az) && finite(bx) && finite(by) && finite(bz) && finite(cx) && finite(cy) &&
          finite(cz))) {
        if (flag) atomicOr(flag, 2);
        return false;
    }
    r.i0 = clamped_cell(fminf(ax, fminf(bx, cx)), g.bx, g.ix, g.cx);
    r.i1 = clamped_cell(fmaxf(ax, fmaxf(bx, cx)), g.bx, g.ix, g.cx);
    r.j0 = clamped_cell(fminf(ay, fminf(by, cy)), g.by, g.iy, g.cy);
    r.j1 = clamped_cell(fmaxf(ay, fmaxf(by, cy)), g.by, g.iy, g.cy);
    r.k0 = clamped_cell(fminf(az, fminf(bz, cz)), g.bz, g.iz, g.cz);
    r.k1 = clamped_cell(fmaxf(az, fmaxf(bz, cz)), g.bz, g.iz, g.cz);
    return true;
}

__global__ __launch_bounds__(BLOCK) void clear_flag_kernel(int *flag) {
    if (threadIdx.x == 0 && blockIdx.x == 0) flag[0] = 0;
}

__global__ __launch_bounds__(BLOCK) void count_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V, int F,
                                                     Grid g, long long *__restrict__ counts, int *flag) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    Range r;
    long long n = 0;
    if (face_range(verts, faces, V, g, f, r, flag))
        n = (long long)(r.i1 - r.i0 + 1) * (long long)(r.j1 - r.j0 + 1) * (long long)(r.k1 - r.k0 + 1);
    counts[f] = n;
}

// pair i: its face is the last f with face_offsets[f] <= i (faces of zero pairs share an offset with their successor and
// are passed over); its cell the (i - face_offsets[f])-th of the face's range, z fastest
__global__ __launch_bounds__(BLOCK) void pairs_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V, int F,
                                                     Grid g, const long long *__restrict__ face_offsets, int n_pairs,
                                                     int *__restrict__ keys, int *__restrict__ pair_face) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_pairs) return;
    int lo = 0, hi = F - 1;                                   // invariant: face_offsets[lo] <= i
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (face_offsets[mid] <= (long long)i)
            lo = mid;
        else
            hi = mid - 1;
    }
    Range r;
    int key = -1;                                             // outside every list: dropped by the lists, never read
    if (face_range(verts, faces, V, g, lo, r, nullptr)) {
        const int local = i - (int)face_offsets[lo];
        const int nk = r.k1 - r.k0 + 1, nj = r.j1 - r.j0 + 1, ni = r.i1 - r.i0 + 1;
        const int di = local / (nj * nk), rem = local - di * (nj * nk);
        const int dj = rem / nk, dk = rem - dj * nk;
        if (di < ni) key = ((r.i0 + di) * g.cy + (r.j0 + dj)) * g.cz + (r.k0 + dk);
    }
    keys[i] = key;
    pair_face[i] = lo;
}

template <bool STATS>
__global__ __launch_bounds__(BLOCK) void query_kernel(const float *__restrict__ points, int N, const float *__restrict__ verts,
                                                     const int *__restrict__ faces, int V, int F, Grid g, double wx, double wy,
                                                     double wz, const int *__restrict__ cell_offsets,
                                                     const int *__restrict__ cell_faces, int *__restrict__ out_face,
                                                     float *__restrict__ out_point, float *__restrict__ out_dist,
                                                     unsigned long long *stats) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (n < N) {
        fx = points[3 * n];
        fy = points[3 * n + 1];
        fz = points[3 * n + 2];
    }
    const bool walk = n < N && finite(fx) && finite(fy) && finite(fz);
    unsigned tests = 0;
    double best = __builtin_huge_val(), bqx = 0.0, bqy = 0.0, bqz = 0.0;
    int bf = -1;
    if (walk)
        shell_walk<STATS>(fx, fy, fz, verts, faces, V, F, g, wx, wy, wz, cell_offsets, cell_faces, __builtin_huge_val(), best, bf,
                          bqx, bqy, bqz, tests);
    if (n < N) {
        const float nan = __builtin_nanf("");
        const bool found = bf >= 0;
        out_face[n] = found ? bf : -1;
        out_point[3 * n] = found ? (float)bqx : nan;
        out_point[3 * n + 1] = found ? (float)bqy : nan;
        out_point[3 * n + 2] = found ? (float)bqz : nan;
        out_dist[n] = found ? (float)sqrt(best) : nan;
    }
    if (STATS) {                                              // integer atomics, once per wave: [0] the tests, [1] 64 x the wave's
        unsigned long long t = tests;                         // longest lane, so [0] / [1] is the share of lane slots that tested
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

// SURFACE SAMPLES.  Subdivision k >= 1 cuts a face into k^2 congruent triangles; sample s of face f, s = 0 .. k^2 - 1:
//   s < k (k + 1) / 2: the upward triangle (i, j), i + j < k, in the order i ascending, then j ascending; numerators
//     (na, nb) = (3 i + 1, 3 j + 1);
//   otherwise the downward triangle (i, j), i + j < k - 1, in the same order; (na, nb) = (3 i + 2, 3 j + 2);
//   nc = 3 k - na - nb; point = fp32(((na a + nb b) + nc c) / (3 k)) per component -- the barycentrics (na, nb, nc) / (3 k), the
//   sub-triangle's centroid; weight = (sqrt(N . N) / 2) / (k k), N = (b - a) x (c - a): an equal-area quadrature rule.
__global__ __launch_bounds__(BLOCK) void sample_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V,
                                                      int n_samples, int k, float *__restrict__ points,
                                                      int *__restrict__ face_of_sample, double *__restrict__ weights, int *flag) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    if (n >= n_samples) return;
    const int kk = k * k, f = n / kk;
    int s = n - f * kk, rows = k, add = 1;
    const int up = k * (k + 1) / 2;
    if (s >= up) {
        s -= up;
        rows = k - 1;
        add = 2;
    }
    int i = 0;
    while (s >= rows - i) {
        s -= rows - i;
        ++i;
    }
    const int na = 3 * i + add, nb = 3 * s + add, nc = 3 * k - na - nb;
    face_of_sample[n] = f;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) {
        atomicOr(flag, 1);
        points[3 * n] = 0.f;
        points[3 * n + 1] = 0.f;
        points[3 * n + 2] = 0.f;
        weights[n] = 0.0;
        return;
    }
    const double ax = (double)verts[3 * a], ay = (double)verts[3 * a + 1], az = (double)verts[3 * a + 2];
    const double bx = (double)verts[3 * b], by = (double)verts[3 * b + 1], bz = (double)verts[3 * b + 2];
    const double cx = (double)verts[3 * c], cy = (double)verts[3 * c + 1], cz = (double)verts[3 * c + 2];
    const double da = (double)na, db = (double)nb, dc = (double)nc, den = (double)(3 * k);
    points[3 * n] = (float)(((da * ax + db * bx) + dc * cx) / den);
    points[3 * n + 1] = (float)(((da * ay + db * by) + dc * cy) / den);
    points[3 * n + 2] = (float)(((da * az + db * bz) + dc * cz) / den);
    double nx, ny, nz;
    cross3(bx - ax, by - ay, bz - az, cx - ax, cy - ay, cz - az, nx, ny, nz);
    weights[n] = (sqrt(dot3(nx, ny, nz, nx, ny, nz)) / 2.0) / (double)kk;
}

static inline bool count_ok(int64_t n) { return n >= 0 && n <= INT_MAX64; }
static inline bool mesh_ok(int64_t V, int64_t F) { return V >= 1 && V <= INT_MAX64 && F >= 1 && 3 * F <= INT_MAX64; }
static inline bool grid_ok(const float *box, const int *cells, Grid &g) {
    static const int some_words = 0;
    return grid_from_args(box, cells, &some_words, g);
}
static inline int64_t n_cells(const Grid &g) { return (int64_t)g.cx * g.cy * g.cz; }
// the list scratch of mvip_mesh_corner_table, rounded up to an even number of words
static inline int64_t list_words(int64_t P, int64_t K) {
    const int64_t w = mvip_mesh_list_scratch_words(P, K);
    return w < 0 ? -1 : (w + 1) / 2 * 2;
}

}  // namespace meshdist
}  // namespace mvip

using namespace mvip;
namespace md = mvip::meshdist;

extern "C" int mvip_mesh_distance_grid_count(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces,
                                             const float *box, const int *cells, int64_t *face_offsets, int64_t *total, int *flag,
                                             void *stream) {
    bitgrid::Grid g;
    if (!md::mesh_ok(n_verts, n_faces) || !md::grid_ok(box, cells, g)) return MVIP_EINVAL;
    if (!verts || !faces || !face_offsets || !total || !flag) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int F = (int)n_faces;
    hipLaunchKernelGGL(md::clear_flag_kernel, dim3(1), dim3(md::BLOCK), 0, s, flag);
    hipLaunchKernelGGL(md::count_kernel, dim3(blocks_for(F, md::BLOCK)), dim3(md::BLOCK), 0, s, verts, faces, (int)n_verts, F, g,
                       (long long *)face_offsets, flag);
    hipLaunchKernelGGL((compact::scan_kernel<long long, 1>), dim3(1), dim3(compact::SCAN_BLOCK), 0, s, (long long *)face_offsets,
                       F, (long long *)total);
    return check_launch();
}

extern "C" int64_t mvip_mesh_distance_grid_scratch_words(int64_t n_pairs, const int *cells) {
    if (!cells || !bitgrid::cells_ok(cells[0], cells[1], cells[2]) || !md::count_ok(n_pairs)) return -1;
    const int64_t lw = md::list_words(n_pairs, (int64_t)cells[0] * cells[1] * cells[2]);
    return lw < 0 ? -1 : lw + 3 * n_pairs + 2;
}

extern "C" int mvip_mesh_distance_grid_fill(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces,
                                            const float *box, const int *cells, const int64_t *face_offsets, int64_t n_pairs,
                                            int *cell_offsets, int *cell_faces, int *scratch, void *stream) {
    bitgrid::Grid g;
    if (!md::mesh_ok(n_verts, n_faces) || !md::grid_ok(box, cells, g) || !md::count_ok(n_pairs)) return MVIP_EINVAL;
    const int64_t K = md::n_cells(g), lw = md::list_words(n_pairs, K);
    if (lw < 0) return MVIP_EINVAL;
    if (!verts || !faces || !face_offsets || !cell_offsets || !scratch || (n_pairs > 0 && !cell_faces)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int P = (int)n_pairs;
    // scratch: the lists' own words | keys [P] | pair_face [P] | items [P] | the lists' flag (a key outside [0, K): only for
    // the faces the count has flagged already)
    int *keys = scratch + lw, *pair_face = keys + n_pairs, *items = pair_face + n_pairs, *list_flag = items + n_pairs;
    if (P > 0)
        hipLaunchKernelGGL(md::pairs_kernel, dim3(blocks_for(P, md::BLOCK)), dim3(md::BLOCK), 0, s, verts, faces, (int)n_verts,
                           (int)n_faces, g, (const long long *)face_offsets, P, keys, pair_face);
    int rc = mvip_mesh_corner_table(keys, n_pairs, K, cell_offsets, items, scratch, list_flag, stream);
    if (rc != MVIP_OK) return rc;
    if (P > 0) rc = mvip_mesh_gather(items, n_pairs, pair_face, n_pairs, cell_faces, stream);
    return rc;
}

extern "C" int mvip_mesh_distance_query(const float *points, int64_t n_points, const float *verts, const int *faces,
                                        int64_t n_verts, int64_t n_faces, const float *box, const int *cells,
                                        const int *cell_offsets, const int *cell_faces, int64_t n_pairs, int *face, float *point,
                                        float *dist, void *stats, void *stream) {
    bitgrid::Grid g;
    if (!md::mesh_ok(n_verts, n_faces) || !md::grid_ok(box, cells, g) || !md::count_ok(n_pairs) || !md::count_ok(n_points) ||
        3 * n_points > md::INT_MAX64)
        return MVIP_EINVAL;
    if (!verts || !faces || !cell_offsets || (n_pairs > 0 && !cell_faces)) return MVIP_EINVAL;
    if (n_points > 0 && (!points || !face || !point || !dist)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    if (stats) hipLaunchKernelGGL(md::clear_stats_kernel, dim3(1), dim3(md::BLOCK), 0, s, (unsigned long long *)stats);
    if (n_points > 0) {
        const double wx = 1.0 / (double)g.ix, wy = 1.0 / (double)g.iy, wz = 1.0 / (double)g.iz;
        const dim3 grid(blocks_for(n_points, md::BLOCK)), block(md::BLOCK);
        if (stats)
            hipLaunchKernelGGL(md::query_kernel<true>, grid, block, 0, s, points, (int)n_points, verts, faces, (int)n_verts,
                               (int)n_faces, g, wx, wy, wz, cell_offsets, cell_faces, face, point, dist, (unsigned long long *)stats);
        else
            hipLaunchKernelGGL(md::query_kernel<false>, grid, block, 0, s, points, (int)n_points, verts, faces, (int)n_verts,
                               (int)n_faces, g, wx, wy, wz, cell_offsets, cell_faces, face, point, dist, (unsigned long long *)nullptr);
    }
    return check_launch();
}

extern "C" int mvip_mesh_sample_faces(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, int k, float *points,
                                      int *face_of_sample, double *weights, int *flag, void *stream) {
    if (!md::count_ok(n_verts) || n_faces < 0 || 3 * n_faces > md::INT_MAX64 || k < 1 || k > md::MAX_SUBDIVISION) return MVIP_EINVAL;
    const int64_t n = n_faces * (int64_t)k * k;
    if (3 * n > md::INT_MAX64 || !flag) return MVIP_EINVAL;
    if (n > 0 && (!verts || !faces || !points || !face_of_sample || !weights || n_verts == 0)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(md::clear_flag_kernel, dim3(1), dim3(md::BLOCK), 0, s, flag);
    if (n > 0)
        hipLaunchKernelGGL(md::sample_kernel, dim3(blocks_for(n, md::BLOCK)), dim3(md::BLOCK), 0, s, verts, faces, (int)n_verts,
                           (int)n, k, points, face_of_sample, weights, flag);
    return check_launch();
}
