// Clean-up of an indexed triangle mesh (beyond the reference, which has no mesh export at all): vertex normals from the
// faces, Taubin smoothing, simplification by vertex clustering (ops.mesh_corner_table / mesh_vertex_normals / mesh_smooth /
// mesh_cluster, mvip_nerf_amd/mesh.py).  THE statement of the definitions; restated for the tests in tests/mesh_ops_numpy.py.
//
// verts [V, 3] fp32, faces [F, 3] int32, counter-clockwise seen from outside.  Corner c = 3 f + k is vertex faces[f, k].
//
// LISTS (the corner table).  For keys [n] int32 in [0, K): offsets [K + 1], items [n]; items[offsets[k] : offsets[k + 1]] are
// the i with keys[i] == k in ASCENDING order.  With keys = the flattened faces and K = V that is the corner table (the corners
// of each vertex); the clustering uses the same lists twice more (members of a cluster: keys = cluster of each vertex; corners
// of a cluster: keys = the faces remapped to clusters).  count (integer atomicAdd) -> exclusive scan (compact::scan_kernel)
// -> fill through an integer cursor (any order) -> rank: every entry counts the entries of its own list below it and moves
// there, so the lists end up ascending whatever order the atomics arrived in.  Every floating-point sum below runs over one
// such list, front to back, in one thread, in fp64: bit-reproducible.  No float atomics.
//
// NORMALS.  n(v) = sum over v's corners c of (p1 - p0) x (p2 - p0), p0 p1 p2 = the vertices of face c / 3 in the face's own
// order (fp64: the fp32 coordinates widened, differences, products, sums, nothing contracted); out = n / sqrt(n . n) per
// component, rounded to fp32; (0, 0, 0) where the list is empty or n . n is not > 0.
//
// SMOOTHING, one pass of weight w: with a, b the two OTHER vertices of corner c's face (a = faces[f, (k + 1) % 3],
// b = faces[f, (k + 2) % 3]) and n the length of v's list, s = sum over the list of (a + b), L = s / (2 n) - v,
// out = v + w L (fp64, rounded to fp32 once per pass); n == 0: out = v.  Taubin: passes of weight lam, mu in turn.
//
// CLUSTERING.  The lattice is the bit grid of csrc/bitgrid_device.h: box origin `origin`, inv = fp32(1 / cell) on all axes,
// (cx, cy, cz) cells; the cell of a vertex is bitgrid::cell_of, a vertex outside the box (NaN, infinite) raises the flag.  The
// bit of every occupied cell is set; cluster id = rank of the bit in linear cell order (compact:: ranks over the words'
// popcounts).  Per cluster (one thread), with C = origin + (i + 0.5, j + 0.5, k + 0.5) * cell in fp64 the cell's centre:
//   mean  m = (sum over the members in ascending vertex order of (p - C)) / n_members;
//   quadric: over the cluster's corner list, face f = c / 3 (a face with two corners in the cluster counts twice),
//     q_i = p_i - C, N = (q1 - q0) x (q2 - q0) (unnormalised: the weight is the squared area), d = -(N . q0), A += N N^T,
//     B += d N; tr = A00 + A11 + A22, cofactors c00 = A11 A22 - A12 A12, c01 = A02 A12 - A01 A22, c02 = A01 A12 - A02 A11,
//     c11 = A00 A22 - A02 A02, c12 = A01 A02 - A00 A12, c22 = A00 A11 - A01 A01, det = A00 c00 + A01 c01 + A02 c02;
//     x = -(cofactor matrix . B) / det, taken iff |det| > 1e-6 (tr / 3)^3 AND cell_of(fp32(C + x)) is the cluster's own cell;
//     otherwise the mean.
//   representative = fp32(C + x) or fp32(C + m); colours: (2 sum + n) / (2 n) in integers over the members.
// Faces: remapped to cluster ids; dropped when two ids are equal; with dedupe also when an EARLIER face has the same directed
// cycle up to rotation (found in the corner list of the face's lowest cluster, which is ascending in the face index).  The
// survivors keep their order (compact:: ranks of the keep flags); clusters no survivor references are dropped and the rest
// renumbered in order (the same ranks over the referenced flags).
#include "bitgrid_device.h"
#include "compact_device.h"
#include "rank_device.h"

namespace mvip {
namespace meshops {

using namespace bitgrid;
using namespace compact;

static const int64_t INT_MAX64 = 2147483647;

__global__ __launch_bounds__(BLOCK) void fill_kernel(int *__restrict__ p, int n, int value) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) p[i] = value;
}

// ---- lists ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void list_count_kernel(const int *__restrict__ keys, int n, int K, int *counts, int *flag) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    if ((unsigned)k >= (unsigned)K) {
        atomicOr(flag, 1);
        return;
    }
    atomicAdd(counts + k, 1);
}

__global__ __launch_bounds__(BLOCK) void list_fill_kernel(const int *__restrict__ keys, int n, int K,
                                                         const int *__restrict__ offsets, int *cursor, int *__restrict__ tmp) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int k = keys[i];
    if ((unsigned)k >= (unsigned)K) return;
    tmp[offsets[k] + atomicAdd(cursor + k, 1)] = i;
}

// entry j of tmp (j below the number of filled entries offsets[K]) moves to its rank inside its own list
__global__ __launch_bounds__(BLOCK) void list_rank_kernel(const int *__restrict__ keys, int n, int K,
                                                         const int *__restrict__ offsets, const int *__restrict__ tmp,
                                                         int *__restrict__ items) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n || j >= offsets[K]) return;
    const int c = tmp[j];
    const int k = keys[c];
    const int lo = offsets[k], hi = offsets[k + 1];
    int r = 0;
    for (int u = lo; u < hi; ++u) r += tmp[u] < c;
    items[lo + r] = c;
}

static int build_lists(const int *keys, int n, int K, int *offsets, int *items, int *scratch, int *flag, hipStream_t s) {
    long long *totals = (long long *)scratch;                  // 2 words
    int *cursor = scratch + 2, *tmp = scratch + 2 + K;
    const dim3 block(BLOCK);
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(K + 1, BLOCK)), block, 0, s, offsets, K + 1, 0);
    if (K > 0) hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(K, BLOCK)), block, 0, s, cursor, K, 0);
    hipLaunchKernelGGL(fill_kernel, dim3(1), block, 0, s, flag, 1, 0);
    if (n > 0) hipLaunchKernelGGL(list_count_kernel, dim3(blocks_for(n, BLOCK)), block, 0, s, keys, n, K, offsets, flag);
    hipLaunchKernelGGL((scan_kernel<int, 1>), dim3(1), dim3(SCAN_BLOCK), 0, s, offsets, K + 1, totals);
    if (n > 0) {
        hipLaunchKernelGGL(list_fill_kernel, dim3(blocks_for(n, BLOCK)), block, 0, s, keys, n, K, (const int *)offsets, cursor, tmp);
        hipLaunchKernelGGL(list_rank_kernel, dim3(blocks_for(n, BLOCK)), block, 0, s, keys, n, K, (const int *)offsets,
                           (const int *)tmp, items);
    }
    return check_launch();
}

// ---- ranks of small counts: rank_device.h ------------------------------------------------------------------------------
struct WordPop {
    const unsigned *w;
    __device__ __forceinline__ int operator()(int i) const { return __popc(w[i]); }
};

// ---- normals and smoothing --------------------------------------------------------------------------------------------
__device__ __forceinline__ void load3(const float *__restrict__ p, int i, double &x, double &y, double &z) {
    x = (double)p[3 * i];
    y = (double)p[3 * i + 1];
    z = (double)p[3 * i + 2];
}

// (p1 - p0) x (p2 - p0)
__device__ __forceinline__ void face_cross(double x0, double y0, double z0, double x1, double y1, double z1, double x2, double y2,
                                           double z2, double &nx, double &ny, double &nz) {
    const double ux = x1 - x0, uy = y1 - y0, uz = z1 - z0, wx = x2 - x0, wy = y2 - y0, wz = z2 - z0;
    nx = uy * wz - uz * wy;
    ny = uz * wx - ux * wz;
    nz = ux * wy - uy * wx;
}

__global__ __launch_bounds__(BLOCK) void normals_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V,
                                                       const int *__restrict__ offsets, const int *__restrict__ corners,
                                                       float *__restrict__ normals) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const int hi = offsets[v + 1];
    for (int j = offsets[v]; j < hi; ++j) {
        const int f = corners[j] / 3;
        double x0, y0, z0, x1, y1, z1, x2, y2, z2, nx, ny, nz;
        load3(verts, faces[3 * f], x0, y0, z0);
        load3(verts, faces[3 * f + 1], x1, y1, z1);
        load3(verts, faces[3 * f + 2], x2, y2, z2);
        face_cross(x0, y0, z0, x1, y1, z1, x2, y2, z2, nx, ny, nz);
        sx += nx;
        sy += ny;
        sz += nz;
    }
    const double n2 = sx * sx + sy * sy + sz * sz;
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (n2 > 0.0 && n2 <= 1.7976931348623157e308) {
        const double len = sqrt(n2);
        ox = (float)(sx / len);
        oy = (float)(sy / len);
        oz = (float)(sz / len);
    }
    normals[3 * v] = ox;
    normals[3 * v + 1] = oy;
    normals[3 * v + 2] = oz;
}

__global__ __launch_bounds__(BLOCK) void smooth_kernel(const float *__restrict__ verts, const int *__restrict__ faces, int V,
                                                      const int *__restrict__ offsets, const int *__restrict__ corners,
                                                      double w, float *__restrict__ out) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int lo = offsets[v], hi = offsets[v + 1];
    const float fx = verts[3 * v], fy = verts[3 * v + 1], fz = verts[3 * v + 2];
    if (hi == lo) {
        out[3 * v] = fx;
        out[3 * v + 1] = fy;
        out[3 * v + 2] = fz;
        return;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = lo; j < hi; ++j) {
        const int c = corners[j];
        const int f = c / 3, k = c - 3 * f;
        const int ka = k == 2 ? 0 : k + 1, kb = k == 0 ? 2 : k - 1;
        double ax, ay, az, bx, by, bz;
        load3(verts, faces[3 * f + ka], ax, ay, az);
        load3(verts, faces[3 * f + kb], bx, by, bz);
        sx += ax + bx;
        sy += ay + by;
        sz += az + bz;
    }
    const double den = 2.0 * (double)(hi - lo);
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    out[3 * v] = (float)(px + w * (sx / den - px));
    out[3 * v + 1] = (float)(py + w * (sy / den - py));
    out[3 * v + 2] = (float)(pz + w * (sz / den - pz));
}

// ---- clustering -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void cluster_mark_kernel(const float *__restrict__ verts, int V, Grid g, unsigned *words,
                                                            int *__restrict__ cell_of_vertex, int *flag) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int l = cell_of(g, verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]);
    cell_of_vertex[v] = l;
    if (l < 0)
        atomicOr(flag, 1);
    else
        atomicOr(words + (l >> 5), 1u << (l & 31));
}

__global__ __launch_bounds__(BLOCK) void cluster_id_kernel(const int *__restrict__ cell_of_vertex, int V,
                                                          const unsigned *__restrict__ words, const int *__restrict__ word_rank,
                                                          int *__restrict__ cluster_of_vertex) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int l = cell_of_vertex[v];
    cluster_of_vertex[v] = l < 0 ? -1 : word_rank[l >> 5] + __popc(words[l >> 5] & ((1u << (l & 31)) - 1u));
}

// out[i] = map[idx[i]] (the faces remapped to clusters); idx was checked against [0, n_map) by the corner table's flag
__global__ __launch_bounds__(BLOCK) void gather_kernel(const int *__restrict__ idx, int n, const int *__restrict__ map, int n_map,
                                                      int *__restrict__ out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int a = idx[i];
    out[i] = (unsigned)a < (unsigned)n_map ? map[a] : -1;
}

__global__ __launch_bounds__(BLOCK) void cluster_place_kernel(
    const float *__restrict__ verts, const unsigned char *__restrict__ colors, const int *__restrict__ faces, Grid g, double cell,
    int K, const int *__restrict__ mem_off, const int *__restrict__ mem, const int *__restrict__ cor_off,
    const int *__restrict__ cor, const int *__restrict__ cell_of_vertex, int quadric, float *__restrict__ rep,
    unsigned char *__restrict__ rep_colors) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= K) return;
    const int m0 = mem_off[k], m1 = mem_off[k + 1];
    if (m1 <= m0) return;                                   // never: a cluster is an occupied cell
    const int l = cell_of_vertex[mem[m0]];
    int ci, cj, ck;
    linear_ijk(l, g.cy, g.cz, ci, cj, ck);
    const double Cx = (double)g.bx + ((double)ci + 0.5) * cell, Cy = (double)g.by + ((double)cj + 0.5) * cell,
                 Cz = (double)g.bz + ((double)ck + 0.5) * cell;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    long long r = 0, gsum = 0, b = 0;
    for (int j = m0; j < m1; ++j) {
        const int v = mem[j];
        double x, y, z;
        load3(verts, v, x, y, z);
        sx += x - Cx;
        sy += y - Cy;
        sz += z - Cz;
        if (colors) {
            r += colors[3 * v];
            gsum += colors[3 * v + 1];
            b += colors[3 * v + 2];
        }
    }
    const double nm = (double)(m1 - m0);
    double px = sx / nm, py = sy / nm, pz = sz / nm;
    if (colors) {
        const long long n = m1 - m0;
        rep_colors[3 * k] = (unsigned char)((2 * r + n) / (2 * n));
        rep_colors[3 * k + 1] = (unsigned char)((2 * gsum + n) / (2 * n));
        rep_colors[3 * k + 2] = (unsigned char)((2 * b + n) / (2 * n));
    }
    if (quadric) {
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        const int hi = cor_off[k + 1];
        for (int j = cor_off[k]; j < hi; ++j) {
            const int f = cor[j] / 3;
            double x0, y0, z0, x1, y1, z1, x2, y2, z2, nx, ny, nz;
            load3(verts, faces[3 * f], x0, y0, z0);
            load3(verts, faces[3 * f + 1], x1, y1, z1);
            load3(verts, faces[3 * f + 2], x2, y2, z2);
            x0 -= Cx; y0 -= Cy; z0 -= Cz;
            x1 -= Cx; y1 -= Cy; z1 -= Cz;
            x2 -= Cx; y2 -= Cy; z2 -= Cz;
            face_cross(x0, y0, z0, x1, y1, z1, x2, y2, z2, nx, ny, nz);
            const double d = -(nx * x0 + ny * y0 + nz * z0);
            a00 += nx * nx; a01 += nx * ny; a02 += nx * nz;
            a11 += ny * ny; a12 += ny * nz; a22 += nz * nz;
            b0 += d * nx; b1 += d * ny; b2 += d * nz;
        }
        const double t3 = (a00 + a11 + a22) / 3.0;
        const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
        const double det = a00 * c00 + a01 * c01 + a02 * c02;
        if (fabs(det) > 1e-6 * (t3 * t3 * t3)) {
            const double qx = -(c00 * b0 + c01 * b1 + c02 * b2) / det, qy = -(c01 * b0 + c11 * b1 + c12 * b2) / det,
                         qz = -(c02 * b0 + c12 * b1 + c22 * b2) / det;
            if (cell_of(g, (float)(Cx + qx), (float)(Cy + qy), (float)(Cz + qz)) == l) {
                px = qx;
                py = qy;
                pz = qz;
            }
        }
    }
    rep[3 * k] = (float)(Cx + px);
    rep[3 * k + 1] = (float)(Cy + py);
    rep[3 * k + 2] = (float)(Cz + pz);
}

// keep[f] and the referenced flags of its clusters; rf = the faces remapped to clusters (every id in [0, K))
__global__ __launch_bounds__(BLOCK) void cluster_keep_kernel(const int *__restrict__ rf, int F, const int *__restrict__ cor_off,
                                                            const int *__restrict__ cor, int dedupe, int *__restrict__ keep,
                                                            int *referenced) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    int a = rf[3 * f], b = rf[3 * f + 1], c = rf[3 * f + 2];
    bool kept = a != b && b != c && a != c;
    if (kept && dedupe) {
        if (b < a && b < c) { const int t = a; a = b; b = c; c = t; }             // the cycle from its lowest id
        else if (c < a && c < b) { const int t = c; c = b; b = a; a = t; }
        const int hi = cor_off[a + 1];
        for (int j = cor_off[a]; j < hi; ++j) {
            const int e = cor[j];
            const int g = e / 3, k = e - 3 * g;
            if (g >= f) break;                                                   // ascending corners: ascending faces
            const int ka = k == 2 ? 0 : k + 1, kb = k == 0 ? 2 : k - 1;
            if (rf[3 * g + ka] == b && rf[3 * g + kb] == c) {                    // rf[e] == a; b, c != a: g is not degenerate
                kept = false;
                break;
            }
        }
    }
    keep[f] = kept;
    if (kept) {
        referenced[a] = 1;
        referenced[b] = 1;
        referenced[c] = 1;
    }
}

__global__ __launch_bounds__(BLOCK) void emit_faces_kernel(const int *__restrict__ rf, int F, const int *__restrict__ keep,
                                                          const int *__restrict__ face_rank, const int *__restrict__ cluster_rank,
                                                          int n_out, int *__restrict__ out) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F || !keep[f]) return;
    const int o = face_rank[f];
    if (o >= n_out) return;
    out[3 * o] = cluster_rank[rf[3 * f]];
    out[3 * o + 1] = cluster_rank[rf[3 * f + 1]];
    out[3 * o + 2] = cluster_rank[rf[3 * f + 2]];
}

__global__ __launch_bounds__(BLOCK) void emit_clusters_kernel(const float *__restrict__ rep, const unsigned char *__restrict__ rep_colors,
                                                             int K, const int *__restrict__ referenced,
                                                             const int *__restrict__ cluster_rank, int n_out, float *__restrict__ out,
                                                             unsigned char *__restrict__ out_colors) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= K || !referenced[k]) return;
    const int o = cluster_rank[k];
    if (o >= n_out) return;
    for (int a = 0; a < 3; ++a) {
        out[3 * o + a] = rep[3 * k + a];
        if (rep_colors) out_colors[3 * o + a] = rep_colors[3 * k + a];
    }
}

__global__ __launch_bounds__(BLOCK) void emit_vertex_ids_kernel(int *cluster_of_vertex, int V, int K,
                                                               const int *__restrict__ referenced,
                                                               const int *__restrict__ cluster_rank) {
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= V) return;
    const int k = cluster_of_vertex[v];
    cluster_of_vertex[v] = (unsigned)k < (unsigned)K && referenced[k] ? cluster_rank[k] : -1;
}

static inline bool count_ok(int64_t n) { return n >= 0 && n <= INT_MAX64; }
// box = (origin[3], inv[3]) with one inv on all axes
static inline bool cluster_grid(const float *box, const int *cells, double cell, Grid &g) {
    static const int some_words = 0;
    if (!grid_from_args(box, cells, &some_words, g)) return false;
    return cell > 0.0 && cell <= 1.7976931348623157e308 && box[3] == box[4] && box[4] == box[5];
}

}  // namespace meshops
}  // namespace mvip

using namespace mvip;
namespace mo = mvip::meshops;

extern "C" int64_t mvip_mesh_list_scratch_words(int64_t n_items, int64_t n_lists) {
    if (!mo::count_ok(n_items) || !mo::count_ok(n_lists) || n_lists + 1 > mo::INT_MAX64) return -1;
    return n_items + n_lists + 2;
}

extern "C" int mvip_mesh_corner_table(const int *keys, int64_t n_items, int64_t n_lists, int *offsets, int *items, int *scratch,
                                      int *flag, void *stream) {
    if (mvip_mesh_list_scratch_words(n_items, n_lists) < 0) return MVIP_EINVAL;
    if (!offsets || !scratch || !flag || (n_items > 0 && (!keys || !items))) return MVIP_EINVAL;
    return mo::build_lists(keys, (int)n_items, (int)n_lists, offsets, items, scratch, flag, as_stream(stream));
}

extern "C" int mvip_mesh_vertex_normals(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces,
                                        const int *offsets, const int *corners, float *normals, void *stream) {
    if (!mo::count_ok(n_verts) || n_faces < 0 || 3 * n_faces > mo::INT_MAX64) return MVIP_EINVAL;
    if (n_verts == 0) return MVIP_OK;
    if (!verts || !offsets || !normals || (n_faces > 0 && (!faces || !corners))) return MVIP_EINVAL;
    hipLaunchKernelGGL(mo::normals_kernel, dim3(blocks_for(n_verts, mo::BLOCK)), dim3(mo::BLOCK), 0, as_stream(stream), verts,
                       faces, (int)n_verts, offsets, corners, normals);
    return check_launch();
}

extern "C" int mvip_mesh_smooth_pass(const float *verts, const int *faces, int64_t n_verts, int64_t n_faces, const int *offsets,
                                     const int *corners, double weight, float *out, void *stream) {
    if (!mo::count_ok(n_verts) || n_faces < 0 || 3 * n_faces > mo::INT_MAX64) return MVIP_EINVAL;
    if (!(fabs(weight) <= 1.7976931348623157e308)) return MVIP_EINVAL;
    if (n_verts == 0) return MVIP_OK;
    if (!verts || !offsets || !out || out == verts || (n_faces > 0 && (!faces || !corners))) return MVIP_EINVAL;
    hipLaunchKernelGGL(mo::smooth_kernel, dim3(blocks_for(n_verts, mo::BLOCK)), dim3(mo::BLOCK), 0, as_stream(stream), verts,
                       faces, (int)n_verts, offsets, corners, weight, out);
    return check_launch();
}

extern "C" int64_t mvip_mesh_rank_groups(int64_t n) {
    if (!mo::count_ok(n)) return -1;
    return (n + mo::PPB - 1) / mo::PPB;
}

extern "C" int mvip_mesh_cluster_assign(const float *verts, int64_t n_verts, const float *box, const int *cells, int *words,
                                        int *cell_of_vertex, int *word_rank, int *wg, int64_t *total, int *cluster_of_vertex,
                                        int *flag, void *stream) {
    bitgrid::Grid g;
    if (!mo::count_ok(n_verts) || !mo::cluster_grid(box, cells, 1.0, g)) return MVIP_EINVAL;
    if (!words || !word_rank || !wg || !total || !flag || (n_verts > 0 && (!verts || !cell_of_vertex || !cluster_of_vertex)))
        return MVIP_EINVAL;
    const int nw = bitgrid::n_words(g.cx, g.cy, g.cz), V = (int)n_verts;
    hipStream_t s = as_stream(stream);
    const dim3 block(mo::BLOCK);
    hipLaunchKernelGGL(mo::fill_kernel, dim3(blocks_for(nw, mo::BLOCK)), block, 0, s, words, nw, 0);
    hipLaunchKernelGGL(mo::fill_kernel, dim3(1), block, 0, s, flag, 1, 0);
    if (V > 0)
        hipLaunchKernelGGL(mo::cluster_mark_kernel, dim3(blocks_for(V, mo::BLOCK)), block, 0, s, verts, V, g, (unsigned *)words,
                           cell_of_vertex, flag);
    mo::ranks<mo::WordPop, 6>(mo::WordPop{(const unsigned *)words}, nw, wg, total, word_rank, s);
    if (V > 0)
        hipLaunchKernelGGL(mo::cluster_id_kernel, dim3(blocks_for(V, mo::BLOCK)), block, 0, s, (const int *)cell_of_vertex, V,
                           (const unsigned *)words, (const int *)word_rank, cluster_of_vertex);
    return check_launch();
}

extern "C" int mvip_mesh_gather(const int *idx, int64_t n, const int *map, int64_t n_map, int *out, void *stream) {
    if (!mo::count_ok(n) || !mo::count_ok(n_map)) return MVIP_EINVAL;
    if (n == 0) return MVIP_OK;
    if (!idx || !out || (n_map > 0 && !map)) return MVIP_EINVAL;
    hipLaunchKernelGGL(mo::gather_kernel, dim3(blocks_for(n, mo::BLOCK)), dim3(mo::BLOCK), 0, as_stream(stream), idx, (int)n, map,
                       (int)n_map, out);
    return check_launch();
}

extern "C" int mvip_mesh_cluster_place(const float *verts, const void *colors, const int *faces, int64_t n_verts, int64_t n_faces,
                                       const float *box, const int *cells, double cell, int64_t n_clusters, const int *mem_offsets,
                                       const int *members, const int *cor_offsets, const int *corners, const int *cell_of_vertex,
                                       int placement, float *rep, void *rep_colors, void *stream) {
    bitgrid::Grid g;
    if (!mo::count_ok(n_verts) || n_faces < 0 || 3 * n_faces > mo::INT_MAX64 || !mo::count_ok(n_clusters) || n_clusters > n_verts ||
        !mo::cluster_grid(box, cells, cell, g) || (placement != 0 && placement != 1))
        return MVIP_EINVAL;
    if (n_clusters == 0) return MVIP_OK;
    if (!verts || !mem_offsets || !members || !cor_offsets || !cell_of_vertex || !rep || (colors && !rep_colors) ||
        (n_faces > 0 && (!faces || !corners)))
        return MVIP_EINVAL;
    hipLaunchKernelGGL(mo::cluster_place_kernel, dim3(blocks_for(n_clusters, mo::BLOCK)), dim3(mo::BLOCK), 0, as_stream(stream),
                       verts, (const unsigned char *)colors, faces, g, cell, (int)n_clusters, mem_offsets, members, cor_offsets,
                       corners, cell_of_vertex, placement, rep, (unsigned char *)rep_colors);
    return check_launch();
}

extern "C" int mvip_mesh_cluster_faces(const int *cluster_faces, int64_t n_faces, int64_t n_clusters, const int *cor_offsets,
                                       const int *corners, int dedupe, int *keep, int *referenced, int *face_wg, int *face_rank,
                                       int *cluster_wg, int *cluster_rank, int64_t *totals, void *stream) {
    if (n_faces < 0 || 3 * n_faces > mo::INT_MAX64 || !mo::count_ok(n_clusters) || (dedupe != 0 && dedupe != 1)) return MVIP_EINVAL;
    if (!totals || !face_wg || !cluster_wg) return MVIP_EINVAL;
    if (n_faces > 0 && (!cluster_faces || !cor_offsets || !corners || !keep || !face_rank)) return MVIP_EINVAL;
    if (n_clusters > 0 && (!referenced || !cluster_rank)) return MVIP_EINVAL;
    const int F = (int)n_faces, K = (int)n_clusters;
    hipStream_t s = as_stream(stream);
    const dim3 block(mo::BLOCK);
    if (K > 0) hipLaunchKernelGGL(mo::fill_kernel, dim3(blocks_for(K, mo::BLOCK)), block, 0, s, referenced, K, 0);
    if (F > 0)
        hipLaunchKernelGGL(mo::cluster_keep_kernel, dim3(blocks_for(F, mo::BLOCK)), block, 0, s, cluster_faces, F, cor_offsets,
                           corners, dedupe, keep, referenced);
    mo::ranks<mo::Flag, 1>(mo::Flag{keep}, F, face_wg, totals, face_rank, s);
    mo::ranks<mo::Flag, 1>(mo::Flag{referenced}, K, cluster_wg, totals + 1, cluster_rank, s);
    return check_launch();
}

extern "C" int mvip_mesh_cluster_emit(const int *cluster_faces, int64_t n_faces, const int *keep, const int *face_rank,
                                      const float *rep, const void *rep_colors, int64_t n_clusters, const int *referenced,
                                      const int *cluster_rank, int64_t n_verts, int64_t n_out_faces, int64_t n_out_verts,
                                      int *cluster_of_vertex, float *out_verts, void *out_colors, int *out_faces, void *stream) {
    if (n_faces < 0 || 3 * n_faces > mo::INT_MAX64 || !mo::count_ok(n_clusters) || !mo::count_ok(n_verts) || n_out_faces < 0 ||
        n_out_faces > n_faces || n_out_verts < 0 || n_out_verts > n_clusters)
        return MVIP_EINVAL;
    if (n_faces > 0 && (!cluster_faces || !keep || !face_rank)) return MVIP_EINVAL;
    if (n_clusters > 0 && (!rep || !referenced || !cluster_rank)) return MVIP_EINVAL;
    if ((n_out_faces > 0 && !out_faces) || (n_out_verts > 0 && (!out_verts || (rep_colors && !out_colors)))) return MVIP_EINVAL;
    if (n_verts > 0 && !cluster_of_vertex) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const dim3 block(mo::BLOCK);
    if (n_out_faces > 0)
        hipLaunchKernelGGL(mo::emit_faces_kernel, dim3(blocks_for(n_faces, mo::BLOCK)), block, 0, s, cluster_faces, (int)n_faces, keep,
                           face_rank, cluster_rank, (int)n_out_faces, out_faces);
    if (n_out_verts > 0)
        hipLaunchKernelGGL(mo::emit_clusters_kernel, dim3(blocks_for(n_clusters, mo::BLOCK)), block, 0, s, rep,
                           (const unsigned char *)rep_colors, (int)n_clusters, referenced, cluster_rank, (int)n_out_verts, out_verts,
                           (unsigned char *)out_colors);
    if (n_verts > 0)
        hipLaunchKernelGGL(mo::emit_vertex_ids_kernel, dim3(blocks_for(n_verts, mo::BLOCK)), block, 0, s, cluster_of_vertex,
                           (int)n_verts, (int)n_clusters, referenced, cluster_rank);
    return check_launch();
}
