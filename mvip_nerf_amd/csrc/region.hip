// Regions: "the surfaces to be inpainted" as a set of cells of a box, lifted from annotated 2D masks and rendered into any
// view (beyond the reference, which takes its masks as given; mvip_nerf_amd/region.py).
//
// The grid is the bit grid of csrc/bitgrid_device.h, the one occupancy uses.  The one difference, and the reason for kernels
// of their own: inside(p) = in the box AND bit set (occupancy's keep(p) is "outside the box OR bit set").
//
//   region_mark:       points [P, 3] -> bits: every point in the box ORs its bit into `words` (in / out: bits already set stay
//                      set).  One thread per point, one vector atomicOr on the word, skipped when a plain load already shows
//                      the bit (bits are only ever set, so a set bit seen is a set bit).  csrc/compact_device.h advertises "no
//                      atomics"; this pass is deterministic for a different reason: OR is commutative and idempotent, so the
//                      words do not depend on the order of execution and the result is reproducible bit for bit.
//   region_accumulate: out[b] = sum over j of (inside(p_bj) ? weights[b, j] : 0), p_bj = rows[b, 0:3] + rows[b, 3:6] * z[b, j]
//                      in the expression of the MLP ray kernels (csrc/mlp_fwd16_kernel.h; the build has -ffp-contract=off).
//                      A select, not a product: a NaN weight outside the region does not reach the sum.  The per-frame pass:
//                      8 B per sample + 44 B per ray + 4 B out, the words stay cached (32 KB at 64^3).  Summation order, fixed:
//                      a ray is summed by one wave; lane t adds the terms j = t, t + 64, t + 128, ... in ascending j into one fp32
//                      accumulator that starts at +0; the 64 lane sums are then added by the six DPP steps of
//                      dpp_incl_sum (row_shr 1, 2, 4, 8, row_bcast 15, row_bcast 31) and lane 63's total is the result.  A ray's
//                      result depends on its own row, depths and weights only: not on B, the chunk or its neighbours.
//                      A wave takes RAYS_PER_WAVE = 4 consecutive rays in turn, each with an accumulator of its own, so that
//                      the loads of four rays are in flight together (one ray per wave: 56 us per 378 x 504 x 128 frame, four:
//                      44 us; a wave that moves 1 KB lives for little but its three dependent round trips).  No LDS, no scratch.
//   region_lookup:     inside(p) of a list of points.
#include "bitgrid_device.h"

namespace mvip {
namespace region {

constexpr int BLOCK = 256;
constexpr int RAYS_PER_WAVE = 4;             // accumulate: consecutive rays per wave, their loads in flight together
constexpr int RAYS_PER_BLOCK = BLOCK / MVIP_WAVE * RAYS_PER_WAVE;

using namespace bitgrid;

__device__ __forceinline__ bool inside(const Grid &g, const unsigned *__restrict__ words, float x, float y, float z) {
    const int l = cell_of(g, x, y, z);
    return l >= 0 && cell_bit(words, l);
}

__global__ __launch_bounds__(BLOCK) void region_mark_kernel(const float *__restrict__ pts, long long P, const Grid g,
                                                           unsigned *words) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= P) return;
    const int l = cell_of(g, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]);
    if (l < 0) return;
    const unsigned bit = 1u << (l & 31);
    if (!(words[l >> 5] & bit)) atomicOr(&words[l >> 5], bit);
}

__global__ __launch_bounds__(BLOCK) void region_accumulate_kernel(const float *__restrict__ rows, const float *__restrict__ z,
                                                                 const float *__restrict__ weights, long long B, int S,
                                                                 const Grid g, const unsigned *__restrict__ words,
                                                                 float *__restrict__ out) {
    const long long b0 = ((long long)blockIdx.x * (BLOCK / MVIP_WAVE) + (threadIdx.x >> 6)) * RAYS_PER_WAVE;   // uniform over the wave
    float o[RAYS_PER_WAVE][3], d[RAYS_PER_WAVE][3], acc[RAYS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < RAYS_PER_WAVE; ++r) {
        const float *row = rows + (b0 + r < B ? b0 + r : 0) * 11;
#pragma unroll
        for (int a = 0; a < 3; ++a) { o[r][a] = row[a]; d[r][a] = row[3 + a]; }
        acc[r] = 0.f;
    }
    for (int j = lane_id(); j < S; j += MVIP_WAVE) {
        float zz[RAYS_PER_WAVE], w[RAYS_PER_WAVE];
#pragma unroll
        for (int r = 0; r < RAYS_PER_WAVE; ++r) {
            const long long s = (b0 + r < B ? b0 + r : 0) * S + j;
            zz[r] = z[s]; w[r] = weights[s];
        }
#pragma unroll
        for (int r = 0; r < RAYS_PER_WAVE; ++r)
            acc[r] += inside(g, words, o[r][0] + d[r][0] * zz[r], o[r][1] + d[r][1] * zz[r], o[r][2] + d[r][2] * zz[r]) ? w[r] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < RAYS_PER_WAVE; ++r) {
        const float total = dpp_wave_sum(acc[r]);
        if (lane_id() == 0 && b0 + r < B) out[b0 + r] = total;
    }
}

__global__ __launch_bounds__(BLOCK) void region_lookup_kernel(const float *__restrict__ pts, long long P, const Grid g,
                                                             const unsigned *__restrict__ words,
                                                             unsigned char *__restrict__ out) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) out[p] = inside(g, words, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]) ? 1 : 0;
}

}  // namespace region
}  // namespace mvip

using namespace mvip;

constexpr int64_t REGION_MAX_POINTS = (int64_t)INT32_MAX * (int64_t)region::BLOCK;

extern "C" int mvip_region_mark(const float *pts, int64_t P, const float *box, const int *cells, int *words, void *stream) {
    bitgrid::Grid g;
    if (P < 0 || P > REGION_MAX_POINTS || !bitgrid::grid_from_args(box, cells, words, g)) return MVIP_EINVAL;
    if (P == 0) return MVIP_OK;
    if (!pts) return MVIP_EINVAL;
    hipLaunchKernelGGL(region::region_mark_kernel, dim3(blocks_for(P, region::BLOCK)), dim3(region::BLOCK), 0,
                       as_stream(stream), pts, (long long)P, g, (unsigned *)words);
    return check_launch();
}

extern "C" int mvip_region_accumulate(const float *rows, const float *z, const float *weights, int64_t B, int S,
                                      const float *box, const int *cells, const int *words, float *out, void *stream) {
    bitgrid::Grid g;
    if (B < 0 || S < 1 || B > (int64_t)INT32_MAX / S || !bitgrid::grid_from_args(box, cells, words, g)) return MVIP_EINVAL;
    if (B == 0) return MVIP_OK;
    if (!rows || !z || !weights || !out) return MVIP_EINVAL;
    hipLaunchKernelGGL(region::region_accumulate_kernel, dim3(blocks_for(B, region::RAYS_PER_BLOCK)), dim3(region::BLOCK), 0,
                       as_stream(stream), rows, z, weights, (long long)B, S, g, (const unsigned *)words, out);
    return check_launch();
}

extern "C" int mvip_region_lookup(const float *pts, int64_t P, const float *box, const int *cells, const int *words, void *out,
                                  void *stream) {
    bitgrid::Grid g;
    if (P < 0 || P > REGION_MAX_POINTS || !bitgrid::grid_from_args(box, cells, words, g)) return MVIP_EINVAL;
    if (P == 0) return MVIP_OK;
    if (!pts || !out) return MVIP_EINVAL;
    hipLaunchKernelGGL(region::region_lookup_kernel, dim3(blocks_for(P, region::BLOCK)), dim3(region::BLOCK), 0,
                       as_stream(stream), pts, (long long)P, g, (const unsigned *)words, (unsigned char *)out);
    return check_launch();
}
