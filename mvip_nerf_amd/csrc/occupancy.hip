// Occupancy-grid empty-space skipping for no-grad renders (beyond the reference: MVIP-NeRF evaluates every sample).
//
// The grid: an axis-aligned box [bmin, bmax] cut into (cx, cy, cz) cells, one bit per cell.  Cell of a point p, per axis in
// fp32: f = floorf((p - bmin) * inv), inv = cells / (bmax - bmin) rounded once on the host; p is inside the box iff
// 0 <= f < c on all three axes (a NaN or infinite coordinate fails the comparison: outside).  Linear cell
// l = (ix * cy + iy) * cz + iz (z fastest), bit l & 31 of 32-bit word l >> 5, unused tail bits zero.
// keep(p) = outside the box, or bit set: a sample is skipped only where the grid says "empty".
// (Conventions shared with mvip_nerf_amd/occupancy.py and the test restatement tests/occupancy_numpy.py.)
//
//   occ_build:   sigma points [cx k + 1, cy k + 1, cz k + 1] -> bits.  Cell (i, j, l) owns points i k .. (i + 1) k on each
//                axis and is occupied iff any of them has !(sigma <= threshold) (NaN counts as occupied).  One thread per
//                cell, one wave ballot per 64 consecutive cells = two words.
//   occ_dilate:  bits -> bits, OR over the 27 cells at Chebyshev distance <= 1 (clipped at the faces).
//   occ_count / occ_scan / occ_emit: order-preserving compaction of the kept samples of a ray chunk, the pattern of
//                csrc/mcubes.hip: workgroup b owns the PPB = 1024 consecutive flat samples s = ray * S + j starting at
//                b * PPB (thread t the samples b * PPB + q * 256 + t, q = 0..3); counts per workgroup from ballot
//                popcounts, one workgroup scans them, the emit pass ranks each kept sample with v_mbcnt inside its wave plus
//                four wave totals in LDS.  The sample's point is formed by the expression of the MLP ray kernels
//                (csrc/mlp_fwd16_kernel.h: row[0] + row[3] * z, ...; the build has -ffp-contract=off), so the points entry
//                point sees the bits the ray entry point would have computed.  No atomics: the output order is ascending s
//                and the result is reproducible bit for bit.  The host reads the total once, to allocate the outputs.
//   occ_scatter: raw_k [K, 4] at idx -> raw [n, 4], zeros elsewhere (a zero-fill pass, then the scatter).
//   occ_lookup:  keep(p) of a list of points.
#include "common.h"

namespace mvip {
namespace occ {

constexpr int BLOCK = 256;
constexpr int PPT = 4;                       // samples per thread
constexpr int PPB = BLOCK * PPT;             // samples per workgroup
constexpr int SCAN_BLOCK = 1024;
constexpr int SCAN_PER_THREAD = 8;

struct Grid {
    float bx, by, bz, ix, iy, iz;
    int cx, cy, cz;
    const unsigned *words;
};

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ bool cell_bit(const unsigned *__restrict__ words, int l) { return (words[l >> 5] >> (l & 31)) & 1u; }

__device__ __forceinline__ bool keep(const Grid &g, float x, float y, float z) {
    const float fx = floorf((x - g.bx) * g.ix), fy = floorf((y - g.by) * g.iy), fz = floorf((z - g.bz) * g.iz);
    const bool inside = fx >= 0.f && fx < (float)g.cx && fy >= 0.f && fy < (float)g.cy && fz >= 0.f && fz < (float)g.cz;
    if (!inside) return true;
    return cell_bit(g.words, ((int)fx * g.cy + (int)fy) * g.cz + (int)fz);
}

__device__ __forceinline__ void cell_ijk(int l, int cy, int cz, int &i, int &j, int &k) {
    const int sx = cy * cz;
    i = l / sx;
    const int r = l - i * sx;
    j = r / cz;
    k = r - j * cz;
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
        cell_ijk(l, cy, cz, i, j, c);
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
        cell_ijk(l, cy, cz, i, j, c);
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
__device__ __forceinline__ bool sample_keep(const Grid &g, const float *__restrict__ rows, const float *__restrict__ z, int s,
                                            int S, const float *&row, float &px, float &py, float &pz) {
    const int ray = s / S;
    row = rows + (long long)ray * 11;
    const float zz = z[s];
    px = row[0] + row[3] * zz; py = row[1] + row[4] * zz; pz = row[2] + row[5] * zz;
    return keep(g, px, py, pz);
}

__global__ __launch_bounds__(BLOCK) void occ_count_kernel(const float *__restrict__ rows, const float *__restrict__ z, int n,
                                                         int S, const Grid g, int *__restrict__ wg_sums,
                                                         unsigned char *__restrict__ mask, float *__restrict__ pts_full) {
    __shared__ int wtot[4];
    int sum = 0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int s = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        bool kp = false;
        if (s < n) {
            const float *row;
            float px, py, pz;
            kp = sample_keep(g, rows, z, s, S, row, px, py, pz);
            if (mask) mask[s] = kp ? 1 : 0;
            if (pts_full) { pts_full[3 * (long long)s] = px; pts_full[3 * (long long)s + 1] = py; pts_full[3 * (long long)s + 2] = pz; }
        }
        sum += __popcll(__ballot(kp));
    }
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) wg_sums[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

__device__ __forceinline__ int wave_incl_i32(int x) {
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (l >= o) x += y;
    }
    return x;
}

// in-place exclusive scan of the G workgroup counts; total[0] = their sum.  One workgroup of 1024 threads, each thread
// owning SCAN_PER_THREAD consecutive counts of an 8192-count chunk.
__global__ __launch_bounds__(SCAN_BLOCK) void occ_scan_kernel(int *__restrict__ wg, int G, long long *__restrict__ total) {
    __shared__ int wsum[2][SCAN_BLOCK / 64];
    int carry = 0;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    int buf = 0;
    for (int c0 = 0; c0 < G; c0 += SCAN_BLOCK * SCAN_PER_THREAD) {
        const int g0 = c0 + threadIdx.x * SCAN_PER_THREAD;
        int sv = 0;
        for (int e = 0; e < SCAN_PER_THREAD; ++e)
            if (g0 + e < G) sv += wg[g0 + e];
        const int iv = wave_incl_i32(sv);
        if (l == 63) wsum[buf][w] = iv;
        __syncthreads();
        int below = 0, tot = 0;
        for (int u = 0; u < SCAN_BLOCK / 64; ++u) {
            const int a = wsum[buf][u];
            if (u < w) below += a;
            tot += a;
        }
        int ev = carry + below + iv - sv;
        for (int e = 0; e < SCAN_PER_THREAD; ++e)
            if (g0 + e < G) {
                const int a = wg[g0 + e];
                wg[g0 + e] = ev;
                ev += a;
            }
        carry += tot;
        buf ^= 1;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

__global__ __launch_bounds__(BLOCK) void occ_emit_kernel(const float *__restrict__ rows, const float *__restrict__ z, int n, int S,
                                                        const Grid g, const int *__restrict__ wg_off, int K,
                                                        int *__restrict__ idx, float *__restrict__ pts,
                                                        float *__restrict__ dirs) {
    __shared__ int wtot[2][4];
    const int w = threadIdx.x >> 6;
    int base = wg_off[blockIdx.x];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int s = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        bool kp = false;
        const float *row = rows;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (s < n) kp = sample_keep(g, rows, z, s, S, row, px, py, pz);
        const unsigned long long m = __ballot(kp);
        int *wt = wtot[q & 1];                       // two buffers in turn: one barrier per round suffices
        if ((threadIdx.x & 63) == 0) wt[w] = __popcll(m);
        __syncthreads();
        const int t0 = wt[0], t1 = wt[1], t2 = wt[2], t3 = wt[3];
        const int id = base + lanes_below(m) + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
        if (kp && id < K) {
            idx[id] = s;
            pts[3 * (long long)id] = px; pts[3 * (long long)id + 1] = py; pts[3 * (long long)id + 2] = pz;
            dirs[3 * (long long)id] = row[8]; dirs[3 * (long long)id + 1] = row[9]; dirs[3 * (long long)id + 2] = row[10];
        }
        base += t0 + t1 + t2 + t3;
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
                                                          unsigned char *__restrict__ out) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) out[p] = keep(g, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]) ? 1 : 0;
}

}  // namespace occ
}  // namespace mvip

using namespace mvip;

static inline bool occ_finite(float x) { return fabsf(x) <= 3.402823466e38f; }
static inline bool occ_cells_ok(int cx, int cy, int cz) {
    return cx >= 1 && cx <= 512 && cy >= 1 && cy <= 512 && cz >= 1 && cz <= 512;
}
static inline int occ_words(int cx, int cy, int cz) { return (int)(((int64_t)cx * cy * cz + 31) / 32); }
static inline bool occ_grid(const float *box, const int *cells, const int *words, occ::Grid &g) {
    if (!box || !cells || !words || !occ_cells_ok(cells[0], cells[1], cells[2])) return false;
    for (int a = 0; a < 6; ++a)
        if (!occ_finite(box[a])) return false;
    if (!(box[3] > 0.f) || !(box[4] > 0.f) || !(box[5] > 0.f)) return false;
    g = occ::Grid{box[0], box[1], box[2], box[3], box[4], box[5], cells[0], cells[1], cells[2], (const unsigned *)words};
    return true;
}
static inline unsigned occ_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

extern "C" int mvip_occupancy_build(const float *sigma, int cx, int cy, int cz, int samples_per_cell, float threshold,
                                    int *words, void *stream) {
    if (!occ_cells_ok(cx, cy, cz) || samples_per_cell < 1 || samples_per_cell > 8) return MVIP_EINVAL;
    if (!(threshold >= 0.f) || !occ_finite(threshold) || !sigma || !words) return MVIP_EINVAL;
    const int64_t N = (int64_t)cx * cy * cz;
    hipLaunchKernelGGL(occ::occ_build_kernel, dim3(occ_blocks(N, occ::BLOCK)), dim3(occ::BLOCK), 0, as_stream(stream), sigma,
                       cx, cy, cz, samples_per_cell, threshold, (unsigned *)words, occ_words(cx, cy, cz));
    return check_launch();
}

extern "C" int mvip_occupancy_dilate(const int *words_in, int cx, int cy, int cz, int *words_out, void *stream) {
    if (!occ_cells_ok(cx, cy, cz) || !words_in || !words_out || words_in == words_out) return MVIP_EINVAL;
    const int64_t N = (int64_t)cx * cy * cz;
    hipLaunchKernelGGL(occ::occ_dilate_kernel, dim3(occ_blocks(N, occ::BLOCK)), dim3(occ::BLOCK), 0, as_stream(stream),
                       (const unsigned *)words_in, cx, cy, cz, (unsigned *)words_out, occ_words(cx, cy, cz));
    return check_launch();
}

extern "C" int64_t mvip_occupancy_groups(int64_t B, int S) {
    if (B < 0 || S < 1 || B > (int64_t)INT32_MAX / S) return -1;
    return (B * S + occ::PPB - 1) / occ::PPB;
}

extern "C" int mvip_occupancy_count(const float *rows, const float *z, int64_t B, int S, const float *box, const int *cells,
                                    const int *words, int *wg, int64_t *total, void *mask, float *pts_full, void *stream) {
    occ::Grid g;
    const int64_t G = mvip_occupancy_groups(B, S);
    if (G < 0 || !occ_grid(box, cells, words, g)) return MVIP_EINVAL;
    if (B == 0) return MVIP_OK;
    if (!rows || !z || !wg || !total) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(occ::occ_count_kernel, dim3((unsigned)G), dim3(occ::BLOCK), 0, s, rows, z, (int)(B * S), S, g, wg,
                       (unsigned char *)mask, pts_full);
    hipLaunchKernelGGL(occ::occ_scan_kernel, dim3(1), dim3(occ::SCAN_BLOCK), 0, s, wg, (int)G, (long long *)total);
    return check_launch();
}

extern "C" int mvip_occupancy_emit(const float *rows, const float *z, int64_t B, int S, const float *box, const int *cells,
                                   const int *words, const int *wg, int64_t K, int *idx, float *pts, float *dirs,
                                   void *stream) {
    occ::Grid g;
    const int64_t G = mvip_occupancy_groups(B, S);
    if (G < 0 || !occ_grid(box, cells, words, g) || K < 0 || K > B * S) return MVIP_EINVAL;
    if (B == 0 || K == 0) return MVIP_OK;
    if (!rows || !z || !wg || !idx || !pts || !dirs) return MVIP_EINVAL;
    hipLaunchKernelGGL(occ::occ_emit_kernel, dim3((unsigned)G), dim3(occ::BLOCK), 0, as_stream(stream), rows, z, (int)(B * S),
                       S, g, wg, (int)K, idx, pts, dirs);
    return check_launch();
}

extern "C" int mvip_scatter_raw(const float *raw_k, const int *idx, int64_t K, int64_t n, float *raw, void *stream) {
    if (K < 0 || n < 0 || K > n || n > (int64_t)INT32_MAX) return MVIP_EINVAL;
    if (n == 0) return MVIP_OK;
    if (!raw || ((uintptr_t)raw & 15) || (K > 0 && (!raw_k || !idx || ((uintptr_t)raw_k & 15)))) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(occ::occ_zero_kernel, dim3(occ_blocks(n, occ::BLOCK)), dim3(occ::BLOCK), 0, s, (float4 *)raw,
                       (long long)n);
    if (K > 0)
        hipLaunchKernelGGL(occ::occ_scatter_kernel, dim3(occ_blocks(K, occ::BLOCK)), dim3(occ::BLOCK), 0, s,
                           (const float4 *)raw_k, idx, (long long)K, (long long)n, (float4 *)raw);
    return check_launch();
}

extern "C" int mvip_occupancy_lookup(const float *pts, int64_t P, const float *box, const int *cells, const int *words,
                                     void *out, void *stream) {
    occ::Grid g;
    if (P < 0 || P > (int64_t)INT32_MAX * (int64_t)occ::BLOCK || !occ_grid(box, cells, words, g)) return MVIP_EINVAL;
    if (P == 0) return MVIP_OK;
    if (!pts || !out) return MVIP_EINVAL;
    hipLaunchKernelGGL(occ::occ_lookup_kernel, dim3(occ_blocks(P, occ::BLOCK)), dim3(occ::BLOCK), 0, as_stream(stream), pts,
                       (long long)P, g, (unsigned char *)out);
    return check_launch();
}
