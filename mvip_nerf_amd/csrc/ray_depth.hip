// Quantile termination depth of a ray: the depth at which the accumulated compositing weight reaches q (q = 0.5: the median
// depth).  Beyond the reference, which renders only the expected depth sum(w z) / sum(w): between two surfaces that mean lies
// where nothing is, a quantile lies on one of them (ops.ray_quantile_depth, run.render_rays(depth_quantiles=...)).
//
// Definition, per ray with S samples in ASCENDING depth z_0 <= ... <= z_{S-1}, weights w_j, and per level q
// (shared word for word with tests/ray_depth_numpy.py; integers and fp64, so no summation order enters):
//   Lq  = (int64) floor((double) q * 2^40)                      a level must have 0 < q < 1 and Lq >= 1
//   W_j = (int64) floor(clamp((double) w_j, 0, 1) * 2^40)       C_j = sum_{i <= j} W_i,  C_{-1} = 0      (S <= 4096: C < 2^52)
//   k   = the smallest j with C_j >= Lq
//   no k:        depth = +inf      (the ray never accumulates q; its disparity 1 / depth is 0)
//   k = S - 1:   depth = z_{S-1}   (the last sample owns an unbounded interval, as in compositing)
//   otherwise:   f = (double)(Lq - C_{k-1}) / (double) W_k;   depth = (float)((double) z_k + f * ((double) z_{k+1} - (double) z_k))
//                (mass w_k lies on [z_k, z_{k+1}], the interval whose length produced alpha_k; -ffp-contract=off: no fma)
//   a ray with any non-finite weight: NaN at every level.  A non-finite z at the crossing propagates by the arithmetic.
//
// Arithmetic: W_j < 2^40 + 1 and C_j < 2^52 are integers that fp64 holds exactly, and fp64 adds them exactly, so the prefix sums
// run as fp64 additions on the DPP scan of common.h and equal the 64-bit integer sums whatever the scan's shape.  The crossing
// sample is the one lane of the ray with C_{k-1} < Lq <= C_k (C_{k-1} = C_k - W_k, exact): no search, and all Q levels come out
// of the one pass over the row.
//
// Shape: one wave per ray, groups of 64 consecutive samples, lane t of group g holding sample k = 64 g + t (a lane past the
// end holds weight 0 and can cross nothing).  z_{k+1} comes from the next lane; lane 63 takes it from a wave-uniform load of
// the next group's first sample.  The loads of four groups are issued together before the first of them is scanned (the scan
// is a chain of dependent steps: 0.087 ms against 0.092 ms with one group's loads at a time, 190,512 x 192, three levels; the
// launch stays at 54 % of the copy rate, profiles/ray_depth.json).  The crossing lane keeps its level's depth in a register; after the last group one lane per
// level stores it (or +inf when no lane crossed, or NaN for a poisoned ray): each of the [B, Q] outputs is stored exactly once.
// No LDS, no scratch, no atomics.  8 B read per sample, 4 Q B written per ray.  A ray's result depends on its own row only.
#include "common.h"
#include <math.h>

namespace mvip {
namespace ray_depth {

constexpr int BLOCK = 256;
constexpr int RAYS_PER_BLOCK = BLOCK / MVIP_WAVE;
constexpr int GROUPS_IN_FLIGHT = 4;
constexpr int MAX_LEVELS = 8;
constexpr int MAX_SAMPLES = 4096;
constexpr double FIX = 1099511627776.0;      // 2^40

struct Levels {
    double L[MAX_LEVELS];                    // Lq as fp64 (exact)
};

__global__ __launch_bounds__(BLOCK) void quantile_depth_kernel(const float *__restrict__ z, const float *__restrict__ weights,
                                                              const long long B, const int S, const Levels lv, const int Q,
                                                              float *__restrict__ depth) {
    const long long b = (long long)blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);      // uniform over the wave
    if (b >= B) return;
    const int lane = lane_id();
    const long long off = b * S;
    const int G = (S + MVIP_WAVE - 1) / MVIP_WAVE;
    float res[MAX_LEVELS];
    unsigned found = 0u;                     // bit q: this lane is level q's crossing sample
    bool bad = false;
    double carry = 0.0;
#pragma unroll
    for (int q = 0; q < MAX_LEVELS; ++q) res[q] = 0.f;

    for (int g0 = 0; g0 < G; g0 += GROUPS_IN_FLIGHT) {
        float zc[GROUPS_IN_FLIGHT], wc[GROUPS_IN_FLIGHT], zfirst[GROUPS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < GROUPS_IN_FLIGHT; ++u) {          // the loads of up to four groups together (g < G is wave-uniform)
            const int g = g0 + u, kc = min(g * MVIP_WAVE + lane, S - 1);
            zc[u] = wc[u] = zfirst[u] = 0.f;
            if (g < G) {
                zc[u] = z[off + kc];
                wc[u] = weights[off + kc];
                zfirst[u] = z[off + min((g + 1) * MVIP_WAVE, S - 1)];          // wave-uniform: the next group's first sample
            }
        }
#pragma unroll
        for (int u = 0; u < GROUPS_IN_FLIGHT; ++u) {
            const int g = g0 + u, k = g * MVIP_WAVE + lane;
            if (g >= G) break;
            const float zn = dpp_from_next(zc[u], zfirst[u]);
            const bool in_ray = k < S;
            bad = bad || (in_ray && !(fabsf(wc[u]) <= 3.402823466e38f));        // NaN, +-inf
            const double wd = fmin(fmax((double)wc[u], 0.0), 1.0);              // NaN: the ray is poisoned anyway
            const double W = in_ray ? floor(wd * FIX) : 0.0;
            const double C = carry + dpp_incl_sum(W);
            const double Cprev = C - W;
            const bool last = k == S - 1;
#pragma unroll
            for (int q = 0; q < MAX_LEVELS; ++q) {
                if (q < Q && Cprev < lv.L[q] && lv.L[q] <= C) {                  // W > 0 here
                    const double f = (lv.L[q] - Cprev) / W;
                    const double zk = (double)zc[u];
                    res[q] = last ? zc[u] : (float)(zk + f * ((double)zn - zk));
                    found |= 1u << q;
                }
            }
            const long long t = __builtin_bit_cast(long long, C);
            const int lo = __builtin_amdgcn_readlane((int)t, 63), hi = __builtin_amdgcn_readlane((int)(t >> 32), 63);
            carry = __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
        }
    }
    const bool poisoned = __ballot(bad) != 0ull;
#pragma unroll
    for (int q = 0; q < MAX_LEVELS; ++q) {
        if (q < Q) {
            const bool mine = (found >> q) & 1u;
            const bool none = __ballot(mine) == 0ull;
            if (mine || (none && lane == 0))
                depth[b * Q + q] = poisoned ? __builtin_nanf("") : (mine ? res[q] : __builtin_inff());
        }
    }
}

}  // namespace ray_depth
}  // namespace mvip

using namespace mvip;

extern "C" int mvip_ray_quantile_depth(const float *z, const float *weights, int64_t B, int S, const float *levels, int Q,
                                       float *depth, void *stream) {
    if (B < 0 || S < 1 || S > ray_depth::MAX_SAMPLES || B > (int64_t)INT32_MAX / S) return MVIP_EINVAL;
    if (Q < 1 || Q > ray_depth::MAX_LEVELS || !levels) return MVIP_EINVAL;
    ray_depth::Levels lv;
    for (int q = 0; q < ray_depth::MAX_LEVELS; ++q) lv.L[q] = 0.0;
    for (int q = 0; q < Q; ++q) {
        if (!(levels[q] > 0.f && levels[q] < 1.f)) return MVIP_EINVAL;           // a NaN fails both
        lv.L[q] = floor((double)levels[q] * ray_depth::FIX);
        if (!(lv.L[q] >= 1.0)) return MVIP_EINVAL;
    }
    if (B == 0) return MVIP_OK;
    if (!z || !weights || !depth) return MVIP_EINVAL;
    hipLaunchKernelGGL(ray_depth::quantile_depth_kernel, dim3(blocks_for(B, ray_depth::RAYS_PER_BLOCK)), dim3(ray_depth::BLOCK), 0,
                       as_stream(stream), z, weights, (long long)B, S, lv, Q, depth);
    return check_launch();
}
