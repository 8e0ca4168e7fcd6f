// Occupancy-grid empty-space skipping for no-grad renders (beyond the reference: MVIP-NeRF evaluates every sample).
//
// The grid is the bit grid of csrc/bitgrid_device.h.  keep(p) = outside the box, or bit set: a sample is skipped only where
// the grid says "empty".
//
//   occ_build:   sigma points [cx k + 1, cy k + 1, cz k + 1] -> bits.  Cell (i, j, l) owns points i k .. (i + 1) k on each
//                axis and is occupied iff any of them has !(sigma <= threshold) (NaN counts as occupied).  One thread per
//                cell, one wave ballot per 64 consecutive cells = two words.
//   occ_dilate:  bits -> bits, OR over the 27 cells at Chebyshev distance <= 1 (clipped at the faces).
//   occ_count / scan / occ_emit: the order-preserving compaction of csrc/compact_device.h over the flat samples
//                s = ray * S + j of a ray chunk, one keep flag per sample.  The sample's point is formed by the expression
//                of the MLP ray kernels (csrc/mlp_fwd16_kernel.h: row[0] + row[3] * z, ...; the build has
//                -ffp-contract=off), so the points entry point sees the bits the ray entry point would have computed.  The
//                output order is ascending s.  The host reads the total once, to allocate the outputs.
//   occ_scatter: raw_k [K, 4] at idx -> raw [n, 4], zeros elsewhere (a zero-fill pass, then the scatter).
//   occ_lookup:  keep(p) of a list of points.
#include "bitgrid_device.h"
#include "compact_device.h"

namespace mvip {
namespace occ {

using namespace bitgrid;
using namespace compact;

__device__ __forceinline__ bool keep(const Grid &g, const unsigned *__restrict__ words, float x, float y, float z) {
    const int l = cell_of(g, x, y, z);
    return l < 0 || cell_bit(words, l);
}

// the wave's 64 cell bits -> words 2 wv, 2 wv + 1 (wv = index of the wave's first cell / 64); cells >= N carry 0
__device__ __forceinline__ void store_wave_bits(bool occ, int l, unsigned *__restrict__ words, int nwords) {
    const unsigned long long m = __ballot(occ);
    const int w0 = (l >> 6) * 2;
    if ((threadIdx.x & 63) == 0) {
        if (w0 < nwords) words[w0] = (unsigned)m;
        if (w0 + 1 < nwords) words[w0 + 1] = (unsigned)(m >> 32);
    }
}

__global__ __launch_bounds__(BLOCK) void occ_build_kernel(const float *__restrict__ sigma, int cx, int cy, int cz, int k,
                                                         float thr, unsigned *__restrict__ words, int nwords) {
    const int N = cx * cy * cz;
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    bool occ = false;
    if (l < N) {
        int i, j, c;
        linear_ijk(l, cy, cz, i, j, c);
        const long long ny = (long long)cy * k + 1, nz = (long long)cz * k + 1;
        for (int a = 0; a <= k; ++a)
            for (int b = 0; b <= k; ++b) {
                const float *r = sigma + ((long long)(i * k + a) * ny + (j * k + b)) * nz + (long long)c * k;
                for (int d = 0; d <= k; ++d) occ = occ || !(r[d] <= thr);
            }
    }
    store_wave_bits(occ, l, words, nwords);
}

__global__ __launch_bounds__(BLOCK) void occ_dilate_kernel(const unsigned *__restrict__ in, int cx, int cy, int cz,
                                                          unsigned *__restrict__ out, int nwords) {
    const int N = cx * cy * cz;
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    bool occ = false;
    if (l < N) {
        int i, j, c;
        linear_ijk(l, cy, cz, i, j, c);
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy) {
                const int x = i + dx, y = j + dy;
                if (x < 0 || x >= cx || y < 0 || y >= cy) continue;
                const int base = (x * cy + y) * cz;
                for (int dz = -1; dz <= 1; ++dz) {
                    const int z = c + dz;
                    if (z >= 0 && z < cz) occ = occ || cell_bit(in, base + z);
                }
            }
    }
    store_wave_bits(occ, l, out, nwords);
}

// point of flat sample s (the source expression of the MLP ray kernels) and its keep bit
__device__ __forceinline__ bool sample_keep(const Grid &g, const unsigned *__restrict__ words, const float *__restrict__ rows,
                                            const float *__restrict__ z, int s, int S, const float *&row, float &px, float &py,
                                            float &pz) {
    const int ray = s / S;
    row = rows + (long long)ray * 11;
    const float zz = z[s];
    px = row[0] + row[3] * zz; py = row[1] + row[4] * zz; pz = row[2] + row[5] * zz;
    return keep(g, words, px, py, pz);
}

__global__ __launch_bounds__(BLOCK) void occ_count_kernel(const float *__restrict__ rows, const float *__restrict__ z, int n,
                                                         int S, const Grid g, const unsigned *__restrict__ words,
                                                         int *__restrict__ wg_sums, unsigned char *__restrict__ mask,
                                                         float *__restrict__ pts_full) {
    __shared__ int wtot[4];
    int sum = 0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int s = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        bool kp = false;
        if (s < n) {
            const float *row;
            float px, py, pz;
            kp = sample_keep(g, words, rows, z, s, S, row, px, py, pz);
            if (mask) mask[s] = kp ? 1 : 0;
            if (pts_full) { pts_full[3 * (long long)s] = px; pts_full[3 * (long long)s + 1] = py; pts_full[3 * (long long)s + 2] = pz; }
        }
        int wt;
        wave_excl_small<1>(kp, wt);
        sum += wt;
    }
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) wg_sums[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

__global__ __launch_bounds__(BLOCK) void occ_emit_kernel(const float *__restrict__ rows, const float *__restrict__ z, int n, int S,
                                                        const Grid g, const unsigned *__restrict__ words,
                                                        const int *__restrict__ wg_off, int K, int *__restrict__ idx,
                                                        float *__restrict__ pts, float *__restrict__ dirs) {
    __shared__ int wtot[2][4];
    int base = wg_off[blockIdx.x];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int s = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        bool kp = false;
        const float *row = rows;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (s < n) kp = sample_keep(g, words, rows, z, s, S, row, px, py, pz);
        int total;
        const int id = base + block_excl_small<1>(kp, wtot[q & 1], total);
        if (kp && id < K) {
            idx[id] = s;
            pts[3 * (long long)id] = px; pts[3 * (long long)id + 1] = py; pts[3 * (long long)id + 2] = pz;
            dirs[3 * (long long)id] = row[8]; dirs[3 * (long long)id + 1] = row[9]; dirs[3 * (long long)id + 2] = row[10];
        }
        base += total;
    }
}

__global__ __launch_bounds__(BLOCK) void occ_zero_kernel(float4 *__restrict__ raw, long long n) {
    const long long s = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (s < n) raw[s] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(BLOCK) void occ_scatter_kernel(const float4 *__restrict__ raw_k, const int *__restrict__ idx,
                                                           long long K, long long n, float4 *__restrict__ raw) {
    const long long j = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= K) return;
    const long long s = idx[j];
    if (s >= 0 && s < n) raw[s] = raw_k[j];
}

__global__ __launch_bounds__(BLOCK) void occ_lookup_kernel(const float *__restrict__ pts, long long P, const Grid g,
                                                          const unsigned *__restrict__ words,
                                                          unsigned char *__restrict__ out) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) out[p] = keep(g, words, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]) ? 1 : 0;
}

}  // namespace occ
}  // namespace mvip

using namespace mvip;

extern "C" int mvip_occupancy_build(const float *sigma, int cx, int cy, int cz, int samples_per_cell, float threshold,
                                    int *words, void *stream) {
    if (!bitgrid::cells_ok(cx, cy, cz) || samples_per_cell < 1 || samples_per_cell > 8) return MVIP_EINVAL;
    if (!(threshold >= 0.f) || !finite(threshold) || !sigma || !words) return MVIP_EINVAL;
    const int64_t N = (int64_t)cx * cy * cz;
    hipLaunchKernelGGL(occ::occ_build_kernel, dim3(blocks_for(N, occ::BLOCK)), dim3(occ::BLOCK), 0, as_stream(stream), sigma,
                       cx, cy, cz, samples_per_cell, threshold, (unsigned *)words, bitgrid::n_words(cx, cy, cz));
    return check_launch();
}

extern "C" int mvip_occupancy_dilate(const int *words_in, int cx, int cy, int cz, int *words_out, void *stream) {
    if (!bitgrid::cells_ok(cx, cy, cz) || !words_in || !words_out || words_in == words_out) return MVIP_EINVAL;
    const int64_t N = (int64_t)cx * cy * cz;
    hipLaunchKernelGGL(occ::occ_dilate_kernel, dim3(blocks_for(N, occ::BLOCK)), dim3(occ::BLOCK), 0, as_stream(stream),
                       (const unsigned *)words_in, cx, cy, cz, (unsigned *)words_out, bitgrid::n_words(cx, cy, cz));
    return check_launch();
}

extern "C" int64_t mvip_occupancy_groups(int64_t B, int S) {
    if (B < 0 || S < 1 || B > (int64_t)INT32_MAX / S) return -1;
    return (B * S + occ::PPB - 1) / occ::PPB;
}

extern "C" int mvip_occupancy_count(const float *rows, const float *z, int64_t B, int S, const float *box, const int *cells,
                                    const int *words, int *wg, int64_t *total, void *mask, float *pts_full, void *stream) {
    bitgrid::Grid g;
    const int64_t G = mvip_occupancy_groups(B, S);
    if (G < 0 || !bitgrid::grid_from_args(box, cells, words, g)) return MVIP_EINVAL;
    if (B == 0) return MVIP_OK;
    if (!rows || !z || !wg || !total) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(occ::occ_count_kernel, dim3((unsigned)G), dim3(occ::BLOCK), 0, s, rows, z, (int)(B * S), S, g,
                       (const unsigned *)words, wg, (unsigned char *)mask, pts_full);
    hipLaunchKernelGGL((compact::scan_kernel<int, 1>), dim3(1), dim3(compact::SCAN_BLOCK), 0, s, wg, (int)G,
                       (long long *)total);
    return check_launch();
}

extern "C" int mvip_occupancy_emit(const float *rows, const float *z, int64_t B, int S, const float *box, const int *cells,
                                   const int *words, const int *wg, int64_t K, int *idx, float *pts, float *dirs,
                                   void *stream) {
    bitgrid::Grid g;
    const int64_t G = mvip_occupancy_groups(B, S);
    if (G < 0 || !bitgrid::grid_from_args(box, cells, words, g) || K < 0 || K > B * S) return MVIP_EINVAL;
    if (B == 0 || K == 0) return MVIP_OK;
    if (!rows || !z || !wg || !idx || !pts || !dirs) return MVIP_EINVAL;
    hipLaunchKernelGGL(occ::occ_emit_kernel, dim3((unsigned)G), dim3(occ::BLOCK), 0, as_stream(stream), rows, z, (int)(B * S),
                       S, g, (const unsigned *)words, wg, (int)K, idx, pts, dirs);
    return check_launch();
}

extern "C" int mvip_scatter_raw(const float *raw_k, const int *idx, int64_t K, int64_t n, float *raw, void *stream) {
    if (K < 0 || n < 0 || K > n || n > (int64_t)INT32_MAX) return MVIP_EINVAL;
    if (n == 0) return MVIP_OK;
    if (!raw || ((uintptr_t)raw & 15) || (K > 0 && (!raw_k || !idx || ((uintptr_t)raw_k & 15)))) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(occ::occ_zero_kernel, dim3(blocks_for(n, occ::BLOCK)), dim3(occ::BLOCK), 0, s, (float4 *)raw,
                       (long long)n);
    if (K > 0)
        hipLaunchKernelGGL(occ::occ_scatter_kernel, dim3(blocks_for(K, occ::BLOCK)), dim3(occ::BLOCK), 0, s,
                           (const float4 *)raw_k, idx, (long long)K, (long long)n, (float4 *)raw);
    return check_launch();
}

extern "C" int mvip_occupancy_lookup(const float *pts, int64_t P, const float *box, const int *cells, const int *words,
                                     void *out, void *stream) {
    bitgrid::Grid g;
    if (P < 0 || P > (int64_t)INT32_MAX * (int64_t)occ::BLOCK || !bitgrid::grid_from_args(box, cells, words, g))
        return MVIP_EINVAL;
    if (P == 0) return MVIP_OK;
    if (!pts || !out) return MVIP_EINVAL;
    hipLaunchKernelGGL(occ::occ_lookup_kernel, dim3(blocks_for(P, occ::BLOCK)), dim3(occ::BLOCK), 0, as_stream(stream), pts,
                       (long long)P, g, (const unsigned *)words, (unsigned char *)out);
    return check_launch();
}
