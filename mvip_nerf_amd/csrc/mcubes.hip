// Indexed, crack-free marching cubes over a dense fp32 grid (beyond the reference: MVIP-NeRF has no mesh export).
//
// grid [nx, ny, nz], C-contiguous, z fastest; point (i, j, k) sits at bmin + (i, j, k) * (bmax - bmin) / (n - 1).
// Every pass partitions the points, and ranks the 0..3 vertices / 0..5 triangles of each, as csrc/compact_device.h says: the
// output order is fixed by the scans and the result is reproducible bit for bit.
//
//   1. mc_classify:  per point the crossing flags of its three owned lattice edges (+x, +y, +z: 0..3 vertices) and, for a
//      cell origin, the 8-bit cube index; one uint16 per point = cube | flags << 8.  Workgroup totals of vertices and
//      triangles (the triangle count of each cube index, read off the table, staged in LDS); a non-finite value raises a
//      device flag with a plain vector store.  With a validity lattice (mvip_mcubes_count_valid) only live cells and the
//      edges around them are classified; the later passes read nothing but the flags, so they are shared.  Normals stay
//      central differences of the grid: within one lattice step of a point that is not valid they read its fill value.
//   2. scan:         one workgroup: exclusive int64 scan of the workgroup totals in place, and the two grand totals.
//      The host reads the totals once, to allocate the outputs (the only synchronisation).
//   3. mc_vertices:  per point its first vertex id (int32), and per crossing edge the position and the normal: the
//      central-difference gradient of sigma at both endpoints (one-sided on the grid's faces), interpolated with the
//      same t as the position, normalised and negated (it points toward decreasing sigma, outward).
//   4. mc_triangles: per cell its triangles, vertex ids found arithmetically: edge e -> axis e >> 2 and corner point
//      (the two other offsets are the bits of e & 3) -> first vertex id of that point + the rank of the axis among the
//      point's crossing edges (popcount of its flags below the axis).  No per-cell id array: nothing indexed at run time
//      lives in registers, so no kernel here uses scratch.
//
// Conventions (shared with tests/mc_numpy.py): corner c = dx + 2 dy + 4 dz; edge e = 4 * axis + r; a corner is inside iff
// v >= iso; t = (iso - v0) / (v1 - v0), p = p0 + t (p1 - p0); vertices ordered by (point, axis), triangles by (cell,
// table slot); the triangle table (mvip_nerf_amd/mesh.py, 256 x 16 int8, -1 terminated) is passed in device memory.
#include "bitgrid_device.h"
#include "compact_device.h"

namespace mvip {
namespace mc {

using namespace compact;
using bitgrid::linear_ijk;

__device__ __forceinline__ int tri_count(const signed char *tab, int cube) {
    int c = 0;
#pragma unroll
    for (int s = 0; s < 5; ++s) c += tab[cube * 16 + 3 * s] >= 0 ? 1 : 0;
    return c;
}

// MASKED (mvip_mcubes_count_valid): `valid` [nx, ny, nz] bytes, non-zero = observed.  A cell is live iff its eight corners are
// valid; a cell that is not live gets cube index 0, and an owned edge keeps its crossing flag only if one of the up to four cells
// around it is live -- so every vertex is referenced by a triangle and every triangle's vertices exist.  Liveness is read off the
// corners directly (the 27 bytes around the point, shared by its seven cells; every index bounded, a point outside the grid
// counts as not valid); the non-finite check applies to valid points only.
template <bool MASKED>
__global__ __launch_bounds__(BLOCK) void mc_classify_kernel(const float *__restrict__ v, const unsigned char *__restrict__ valid,
                                                           int nx, int ny, int nz, float iso,
                                                           const signed char *__restrict__ table,
                                                           unsigned short *__restrict__ flags,
                                                           long long *__restrict__ wg_sums, unsigned *__restrict__ nonfinite) {
    __shared__ int counts[256];
    __shared__ int wtot[2][4];                   // [vertices | triangles][wave]
    counts[threadIdx.x] = tri_count(table, threadIdx.x);
    __syncthreads();
    const int N = nx * ny * nz, sx = ny * nz, sy = nz;
    int vsum = 0, tsum = 0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int n = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        int nv = 0, nt = 0;
        if (n < N) {
            int i, j, k;
            linear_ijk(n, ny, nz, i, j, k);
            const float v0 = v[n];
            if (!finite(v0) && (!MASKED || valid[n] != 0)) *nonfinite = 1u;      // NaN or +-inf
            const bool xi = i + 1 < nx, yi = j + 1 < ny, zi = k + 1 < nz;
            const unsigned c0 = v0 >= iso;
            const unsigned c1 = xi ? (v[n + sx] >= iso) : c0;
            const unsigned c2 = yi ? (v[n + sy] >= iso) : c0;
            const unsigned c4 = zi ? (v[n + 1] >= iso) : c0;
            unsigned mask = (c0 ^ c1) | ((c0 ^ c2) << 1) | ((c0 ^ c4) << 2);
            unsigned cube = 0;
            if (xi && yi && zi) {
                const unsigned c3 = v[n + sx + sy] >= iso, c5 = v[n + sx + 1] >= iso;
                const unsigned c6 = v[n + sy + 1] >= iso, c7 = v[n + sx + sy + 1] >= iso;
                cube = c0 | (c1 << 1) | (c2 << 2) | (c3 << 3) | (c4 << 4) | (c5 << 5) | (c6 << 6) | (c7 << 7);
            }
            if constexpr (MASKED) {
                // ok(dx, dy, dz): the point at that offset (-1..1 each) exists and is valid
                auto ok = [&](int dx, int dy, int dz) -> unsigned {
                    const int a = i + dx, b = j + dy, c = k + dz;
                    if (a < 0 || a >= nx || b < 0 || b >= ny || c < 0 || c >= nz) return 0u;
                    return valid[n + dx * sx + dy * sy + dz] != 0 ? 1u : 0u;
                };
                // live(a, b, c): the cell whose origin is at offset (a, b, c) (-1 or 0 each) has eight valid corners
                auto live = [&](int a, int b, int c) -> unsigned {
                    return ok(a, b, c) & ok(a + 1, b, c) & ok(a, b + 1, c) & ok(a + 1, b + 1, c) & ok(a, b, c + 1) &
                           ok(a + 1, b, c + 1) & ok(a, b + 1, c + 1) & ok(a + 1, b + 1, c + 1);
                };
                const unsigned l000 = live(0, 0, 0), l0m0 = live(0, -1, 0), l00m = live(0, 0, -1), l0mm = live(0, -1, -1);
                const unsigned lm00 = live(-1, 0, 0), lm0m = live(-1, 0, -1), lmm0 = live(-1, -1, 0);
                const unsigned ex = l000 | l0m0 | l00m | l0mm, ey = l000 | lm00 | l00m | lm0m, ez = l000 | lm00 | l0m0 | lmm0;
                mask &= ex | (ey << 1) | (ez << 2);
                cube = l000 ? cube : 0u;
            }
            flags[n] = (unsigned short)(cube | (mask << 8));
            nv = __popc(mask);
            nt = counts[cube];
        }
        int wv, wt;
        wave_excl_small<3>(nv, wv);
        wave_excl_small<3>(nt, wt);
        vsum += wv;
        tsum += wt;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wtot[0][w] = vsum; wtot[1][w] = tsum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        wg_sums[2 * (long long)blockIdx.x] = (long long)wtot[0][0] + wtot[0][1] + wtot[0][2] + wtot[0][3];
        wg_sums[2 * (long long)blockIdx.x + 1] = (long long)wtot[1][0] + wtot[1][1] + wtot[1][2] + wtot[1][3];
    }
}

// d sigma / d axis at point n (index ii of nn along the axis, stride s, spacing h): central inside, one-sided on a face
__device__ __forceinline__ float grad1(const float *__restrict__ v, int n, int ii, int nn, int s, float h) {
    const int lo = ii > 0 ? 1 : 0, hi = ii + 1 < nn ? 1 : 0;
    return (v[n + hi * s] - v[n - lo * s]) / ((float)(hi + lo) * h);
}

__global__ __launch_bounds__(BLOCK) void mc_vertices_kernel(const float *__restrict__ v, int nx, int ny, int nz, float iso,
                                                           float x0, float y0, float z0, float hx, float hy, float hz,
                                                           const unsigned short *__restrict__ flags,
                                                           const long long *__restrict__ wg_off, long long V,
                                                           int *__restrict__ vid, float *__restrict__ verts,
                                                           float *__restrict__ normals) {
    __shared__ int wtot[2][4];
    const int N = nx * ny * nz, sx = ny * nz, sy = nz;
    long long base = wg_off[2 * (long long)blockIdx.x];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int n = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        const unsigned mask = n < N ? (unsigned)(flags[n] >> 8) : 0u;
        int total;
        const int pre = block_excl_small<3>(__popc(mask), wtot[q & 1], total);
        if (n < N) {
            long long id = base + pre;
            vid[n] = (int)id;
            if (mask) {
                int i, j, k;
                linear_ijk(n, ny, nz, i, j, k);
                const float v0 = v[n];
                const float px = x0 + (float)i * hx, py = y0 + (float)j * hy, pz = z0 + (float)k * hz;
                const float g0x = grad1(v, n, i, nx, sx, hx), g0y = grad1(v, n, j, ny, sy, hy), g0z = grad1(v, n, k, nz, 1, hz);
                for (int a = 0; a < 3; ++a) {
                    if (!((mask >> a) & 1u)) continue;
                    const int da = a == 0, db = a == 1, dc = a == 2;
                    const int i1 = i + da, j1 = j + db, k1 = k + dc;
                    const int n1 = n + da * sx + db * sy + dc;
                    const float v1 = v[n1];
                    const float t = (iso - v0) / (v1 - v0);
                    const float qx = x0 + (float)i1 * hx, qy = y0 + (float)j1 * hy, qz = z0 + (float)k1 * hz;
                    const float g1x = grad1(v, n1, i1, nx, sx, hx), g1y = grad1(v, n1, j1, ny, sy, hy),
                                g1z = grad1(v, n1, k1, nz, 1, hz);
                    const float gx = g0x + t * (g1x - g0x), gy = g0y + t * (g1y - g0y), gz = g0z + t * (g1z - g0z);
                    const float len = sqrtf(gx * gx + gy * gy + gz * gz);
                    if (id < V) {
                        verts[3 * id + 0] = px + t * (qx - px);
                        verts[3 * id + 1] = py + t * (qy - py);
                        verts[3 * id + 2] = pz + t * (qz - pz);
                        normals[3 * id + 0] = len > 0.f ? -gx / len : 0.f;
                        normals[3 * id + 1] = len > 0.f ? -gy / len : 0.f;
                        normals[3 * id + 2] = len > 0.f ? -gz / len : 0.f;
                    }
                    ++id;
                }
            }
        }
        base += total;
    }
}

__global__ __launch_bounds__(BLOCK) void mc_triangles_kernel(int nx, int ny, int nz, const signed char *__restrict__ table,
                                                            const unsigned short *__restrict__ flags,
                                                            const int *__restrict__ vid,
                                                            const long long *__restrict__ wg_off, long long F,
                                                            int *__restrict__ faces) {
    __shared__ int4 tab4[256];
    __shared__ int wtot[2][4];
    tab4[threadIdx.x] = reinterpret_cast<const int4 *>(table)[threadIdx.x];
    __syncthreads();
    const signed char *tab = reinterpret_cast<const signed char *>(tab4);
    const int N = nx * ny * nz, sx = ny * nz, sy = nz;
    long long base = wg_off[2 * (long long)blockIdx.x + 1];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int n = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        const int cube = n < N ? (int)(flags[n] & 0xffu) : 0;
        const int nt = tri_count(tab, cube);
        int total;
        const int pre = block_excl_small<3>(nt, wtot[q & 1], total);
        for (int s = 0; s < nt; ++s) {
            const long long f = base + pre + s;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int e = tab[cube * 16 + 3 * s + c];
                const int a = e >> 2, r1 = e & 1, r2 = (e >> 1) & 1;
                const int dx = a == 0 ? 0 : r1, dy = a == 1 ? 0 : (a == 0 ? r1 : r2), dz = a == 2 ? 0 : r2;
                const int m = n + dx * sx + dy * sy + dz;
                const int id = vid[m] + __popc((unsigned)(flags[m] >> 8) & ((1u << a) - 1u));
                if (f < F) faces[3 * f + c] = id;
            }
        }
        base += total;
    }
}

}  // namespace mc
}  // namespace mvip

using namespace mvip;

static inline bool mc_shape_ok(int nx, int ny, int nz) {
    return nx >= 2 && nx <= 768 && ny >= 2 && ny <= 768 && nz >= 2 && nz <= 768;
}

extern "C" int64_t mvip_mcubes_groups(int nx, int ny, int nz) {
    if (!mc_shape_ok(nx, ny, nz)) return -1;
    return ((int64_t)nx * ny * nz + mc::PPB - 1) / mc::PPB;
}

extern "C" int mvip_mcubes_count(const float *grid, int nx, int ny, int nz, float iso, const void *tri_table, void *flags,
                                 int64_t *wg, int64_t *totals, void *stream) {
    if (!mc_shape_ok(nx, ny, nz) || !(iso > 0.f) || !finite(iso)) return MVIP_EINVAL;
    if (!grid || !tri_table || !flags || !wg || !totals) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int64_t G = mvip_mcubes_groups(nx, ny, nz);
    zero_words(totals + 2, 2, s);                               // totals[2]: the non-finite flag
    hipLaunchKernelGGL(mc::mc_classify_kernel<false>, dim3((unsigned)G), dim3(mc::BLOCK), 0, s, grid,
                       (const unsigned char *)nullptr, nx, ny, nz, iso, (const signed char *)tri_table, (unsigned short *)flags,
                       (long long *)wg, (unsigned *)(totals + 2));
    hipLaunchKernelGGL((compact::scan_kernel<long long, 2>), dim3(1), dim3(compact::SCAN_BLOCK), 0, s, (long long *)wg,
                       (int)G, (long long *)totals);
    return check_launch();
}

extern "C" int mvip_mcubes_count_valid(const float *grid, const void *valid, int nx, int ny, int nz, float iso,
                                       const void *tri_table, void *flags, int64_t *wg, int64_t *totals, void *stream) {
    if (!mc_shape_ok(nx, ny, nz) || !(iso > 0.f) || !finite(iso)) return MVIP_EINVAL;
    if (!grid || !valid || !tri_table || !flags || !wg || !totals) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int64_t G = mvip_mcubes_groups(nx, ny, nz);
    zero_words(totals + 2, 2, s);                               // totals[2]: the non-finite flag
    hipLaunchKernelGGL(mc::mc_classify_kernel<true>, dim3((unsigned)G), dim3(mc::BLOCK), 0, s, grid,
                       (const unsigned char *)valid, nx, ny, nz, iso, (const signed char *)tri_table, (unsigned short *)flags,
                       (long long *)wg, (unsigned *)(totals + 2));
    hipLaunchKernelGGL((compact::scan_kernel<long long, 2>), dim3(1), dim3(compact::SCAN_BLOCK), 0, s, (long long *)wg,
                       (int)G, (long long *)totals);
    return check_launch();
}

extern "C" int mvip_mcubes_emit(const float *grid, int nx, int ny, int nz, float iso, float x0, float y0, float z0, float x1,
                                float y1, float z1, const void *tri_table, const void *flags, const int64_t *wg,
                                int64_t n_verts, int64_t n_tris, int *vid, float *verts, float *normals, int *faces,
                                void *stream) {
    if (!mc_shape_ok(nx, ny, nz) || !(iso > 0.f) || !finite(iso)) return MVIP_EINVAL;
    if (!finite(x0) || !finite(y0) || !finite(z0) || !finite(x1) || !finite(y1) || !finite(z1) ||
        !(x0 < x1) || !(y0 < y1) || !(z0 < z1)) return MVIP_EINVAL;
    if (n_verts < 0 || n_tris < 0 || n_verts > 3 * (int64_t)nx * ny * nz || n_tris > (int64_t)INT32_MAX) return MVIP_EINVAL;
    if (n_verts == 0 && n_tris == 0) return MVIP_OK;
    if (!grid || !tri_table || !flags || !wg || !vid || !verts || !normals || (n_tris > 0 && !faces)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int64_t G = mvip_mcubes_groups(nx, ny, nz);
    const float hx = (x1 - x0) / (float)(nx - 1), hy = (y1 - y0) / (float)(ny - 1), hz = (z1 - z0) / (float)(nz - 1);
    hipLaunchKernelGGL(mc::mc_vertices_kernel, dim3((unsigned)G), dim3(mc::BLOCK), 0, s, grid, nx, ny, nz, iso, x0, y0, z0,
                       hx, hy, hz, (const unsigned short *)flags, (const long long *)wg, (long long)n_verts, vid, verts,
                       normals);
    if (n_tris > 0)
        hipLaunchKernelGGL(mc::mc_triangles_kernel, dim3((unsigned)G), dim3(mc::BLOCK), 0, s, nx, ny, nz,
                           (const signed char *)tri_table, (const unsigned short *)flags, (const int *)vid,
                           (const long long *)wg, (long long)n_tris, faces);
    return check_launch();
}
