// Ray distortion loss (mip-NeRF 360, eq. 15): a per-ray penalty on how spread out the compositing weights are along the ray
// (beyond the reference, which has no regulariser of this kind; ops.distortion_loss, run.render_rays(distortion=True)).
//
// Definition, per ray with S samples in ASCENDING depth z_0 <= ... <= z_{S-1}, weights w_j, near = row[6], far = row[7]
// (conventions shared with tests/distortion_numpy.py):
//   s_j = (z_j - near) / (far - near), or with lindisp (1/z_j - 1/near) / (1/far - 1/near): every operation one correctly rounded
//         fp32 operation in that order (the build has -ffp-contract=off; fp32 division is correctly rounded).
//   sample j < S-1 owns [s_j, s_{j+1}]: m_j = 0.5 * (s_j + s_{j+1}), d_j = s_{j+1} - s_j; the last sample owns a point,
//         m_{S-1} = s_{S-1}, d_{S-1} = 0 (compositing gives it the 1e10 background interval).
//   L     = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_j w_j^2 d_j
//   dL/dw_k = 2 sum_j w_j |m_k - m_j| + (2/3) w_k d_k          (gradient to the weights only)
//
// Arithmetic: sums of non-negative terms only, never a difference of prefix sums (m_k W_{<k} - WM_{<k} cancels on peaked rays):
//   D_k = sum_{j<k} w_j (m_k - m_j) = D_{k-1} + (m_k - m_{k-1}) * W_{<k}        W_{<k} = sum_{j<k} w_j       (ascending sweep)
//   U_k = sum_{j>k} w_j (m_j - m_k) = U_{k+1} + (m_{k+1} - m_k) * W_{>k}        W_{>k} = sum_{j>k} w_j       (descending sweep)
//   L = sum_k w_k * (2 * D_k + (w_k * d_k) * (1/3))          dL/dw_k = 2 * (D_k + U_k) + ((2/3) * w_k) * d_k
// (m is non-decreasing because every operation of s and m is monotone, so the m differences are the |.| of the definition.)
//
// Summation order, fixed: a ray is handled by one wave in groups of 64 consecutive samples, lane t of group g holding sample
// k = 64 g + t.  A lane past the end holds a copy of the last sample's point with weight +0 (its terms are +0).
//   ascending, g = 0, 1, ...:  P = dpp_incl_sum(w) (row_shr 1, 2, 4, 8, row_bcast 15, row_bcast 31);  W_{<k} = carryW + P_{t-1}
//       (lane 0: carryW + 0);  E_k = (m_k - m_{k-1}) * W_{<k} (m_{k-1} of lane 0 is the previous group's lane 63; E_0 = 0);
//       D_k = carryD + dpp_incl_sum(E)_t;  then carryW += P_63, carryD = D at lane 63.  Carries start at +0.
//       The loss terms of lane t are added over the groups in ascending g into one fp32 accumulator that starts at +0; the 64 lane
//       sums are added by dpp_incl_sum and lane 63's total is the loss.
//   descending, g = G-1, ..., 0 (only when a gradient is asked for): the mirror image with an inclusive SUFFIX sum Q over the lanes:
//       row_shl 1, 2, 4, 8 inside the rows of 16, then with the row totals t1, t2, t3 read from lanes 16, 32, 48: row 2 += t3,
//       row 1 += (t2 + t3), row 0 += (t1 + (t2 + t3)).  W_{>k} = carryW + Q_{t+1} (lane 63: carryW + 0);
//       F_k = (m_{k+1} - m_k) * W_{>k};  U_k = carryU + suffix(F)_t;  then carryW += Q_0, carryU = U at lane 0.
// A ray's result depends on its own row, depths and weights only: not on B, the chunk or its neighbours.  The loss of a call
// without a gradient is the loss of a call with one, bit for bit (the same ascending sweep).
//
// Shape: a wave takes RAYS_PER_WAVE = 4 consecutive rays together so that the loads of four rays are in flight (as
// region_accumulate does).  No LDS, no scratch, no atomics.  D_k of every group but the last waits for the descending sweep
// in the gradient row itself: the lane that wrote grad[b, k] = D_k is the lane that reads it back and overwrites it with the
// gradient (program order of one thread; the row was written a moment ago, the read is an L2 hit); the last group's D, m, d and w
// stay in registers, so S <= 64 makes no round trip and reads its inputs once.  8 B read + 4 B written per sample.
#include "common.h"

namespace mvip {
namespace distortion {

constexpr int BLOCK = 256;
constexpr int RAYS_PER_WAVE = 4;
constexpr int RAYS_PER_BLOCK = BLOCK / MVIP_WAVE * RAYS_PER_WAVE;

template <bool LINDISP>
__device__ __forceinline__ float norm_dist(float z, float a, float den) { return ((LINDISP ? 1.f / z : z) - a) / den; }

__device__ __forceinline__ float lane_value(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// inclusive suffix sum over the 64 lanes (lane l gets the sum over lanes >= l); the order is the file header's
__device__ __forceinline__ float dpp_incl_suffix_sum(float v) {
    v += dpp_f32<0x101>(0.f, v);
    v += dpp_f32<0x102>(0.f, v);
    v += dpp_f32<0x104>(0.f, v);
    v += dpp_f32<0x108>(0.f, v);
    const float t1 = lane_value(v, 16), t2 = lane_value(v, 32), t3 = lane_value(v, 48);
    const float t23 = t2 + t3, t123 = t1 + t23;
    const int row = lane_id() >> 4;
    if (row < 3) v += row == 0 ? t123 : row == 1 ? t23 : t3;
    return v;
}

// one group of one ray: normalised midpoint m, width d and weight w (0 past the end) of sample min(k, S - 1)
template <bool LINDISP>
__device__ __forceinline__ void interval(float zc, float zn, float wc, bool in_ray, float a, float den, float &m, float &d, float &w) {
    const float s = norm_dist<LINDISP>(zc, a, den), sn = norm_dist<LINDISP>(zn, a, den);
    m = 0.5f * (s + sn);
    d = sn - s;
    w = in_ray ? wc : 0.f;
}

template <bool LINDISP>
__global__ __launch_bounds__(BLOCK) void distortion_loss_kernel(const float *__restrict__ rows, int ncols, const float *__restrict__ z,
                                                               const float *__restrict__ weights, long long B, int S,
                                                               float *__restrict__ loss, float *grad) {
    const long long b0 = ((long long)blockIdx.x * (BLOCK / MVIP_WAVE) + (threadIdx.x >> 6)) * RAYS_PER_WAVE;   // uniform over the wave
    if (b0 >= B) return;
    const int lane = lane_id();
    const int G = (S + MVIP_WAVE - 1) / MVIP_WAVE;
    long long off[RAYS_PER_WAVE];
    float a[RAYS_PER_WAVE], den[RAYS_PER_WAVE];
    bool live[RAYS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < RAYS_PER_WAVE; ++r) {
        live[r] = b0 + r < B;
        const long long b = live[r] ? b0 + r : b0;
        const float near = rows[b * ncols + 6], far = rows[b * ncols + 7];
        a[r] = LINDISP ? 1.f / near : near;
        den[r] = (LINDISP ? 1.f / far : far) - a[r];
        off[r] = b * S;
    }

    float acc[RAYS_PER_WAVE], cW[RAYS_PER_WAVE], cD[RAYS_PER_WAVE], cM[RAYS_PER_WAVE];
    float m[RAYS_PER_WAVE], d[RAYS_PER_WAVE], w[RAYS_PER_WAVE], D[RAYS_PER_WAVE];      // of the group at hand; the last group's survive
#pragma unroll
    for (int r = 0; r < RAYS_PER_WAVE; ++r) acc[r] = cW[r] = cD[r] = cM[r] = 0.f;

    for (int g = 0; g < G; ++g) {
        const int k = g * MVIP_WAVE + lane, kc = min(k, S - 1), kn = min(k + 1, S - 1);
        float zc[RAYS_PER_WAVE], zn[RAYS_PER_WAVE], wc[RAYS_PER_WAVE];
#pragma unroll
        for (int r = 0; r < RAYS_PER_WAVE; ++r) { zc[r] = z[off[r] + kc]; zn[r] = z[off[r] + kn]; wc[r] = weights[off[r] + kc]; }
#pragma unroll
        for (int r = 0; r < RAYS_PER_WAVE; ++r) {
            interval<LINDISP>(zc[r], zn[r], wc[r], k < S, a[r], den[r], m[r], d[r], w[r]);
            const float P = dpp_incl_sum(w[r]);
            const float Wlt = cW[r] + dpp_from_prev(P, 0.f);
            const float mp = dpp_from_prev(m[r], g == 0 ? m[r] : cM[r]);
            const float E = (m[r] - mp) * Wlt;
            D[r] = cD[r] + dpp_incl_sum(E);
            acc[r] += w[r] * (2.f * D[r] + (w[r] * d[r]) * (1.f / 3.f));
            cW[r] += lane_value(P, 63);
            cD[r] = lane_value(D[r], 63);
            cM[r] = lane_value(m[r], 63);
            if (grad && g < G - 1 && live[r]) grad[off[r] + k] = D[r];       // k < S in every group but the last
        }
    }
#pragma unroll
    for (int r = 0; r < RAYS_PER_WAVE; ++r) {
        const float total = dpp_wave_sum(acc[r]);
        if (lane == 0 && live[r]) loss[b0 + r] = total;
    }
    if (!grad) return;

#pragma unroll
    for (int r = 0; r < RAYS_PER_WAVE; ++r) cW[r] = cD[r] = cM[r] = 0.f;      // now the carries of W_{>k}, U and m_{k+1}
    for (int g = G - 1; g >= 0; --g) {
        const int k = g * MVIP_WAVE + lane;
        if (g < G - 1) {            // uniform; the last group is still in registers
            float zc[RAYS_PER_WAVE], zn[RAYS_PER_WAVE], wc[RAYS_PER_WAVE];
#pragma unroll
            for (int r = 0; r < RAYS_PER_WAVE; ++r) {
                zc[r] = z[off[r] + k]; zn[r] = z[off[r] + k + 1]; wc[r] = weights[off[r] + k];       // k + 1 < S here
                D[r] = live[r] ? grad[off[r] + k] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < RAYS_PER_WAVE; ++r) interval<LINDISP>(zc[r], zn[r], wc[r], true, a[r], den[r], m[r], d[r], w[r]);
        }
#pragma unroll
        for (int r = 0; r < RAYS_PER_WAVE; ++r) {
            const float Q = dpp_incl_suffix_sum(w[r]);
            const float Wgt = cW[r] + dpp_from_next(Q, 0.f);
            const float mn = dpp_from_next(m[r], g == G - 1 ? m[r] : cM[r]);
            const float F = (mn - m[r]) * Wgt;
            const float U = cD[r] + dpp_incl_suffix_sum(F);
            cW[r] += lane_value(Q, 0);
            cD[r] = lane_value(U, 0);
            cM[r] = lane_value(m[r], 0);
            if (live[r] && k < S) grad[off[r] + k] = 2.f * (D[r] + U) + ((2.f / 3.f) * w[r]) * d[r];
        }
    }
}

}  // namespace distortion
}  // namespace mvip

using namespace mvip;

extern "C" int mvip_distortion_loss(const float *rows, int ncols, const float *z, const float *weights, int64_t B, int S,
                                    int lindisp, float *loss, float *grad, void *stream) {
    if (B < 0 || S < 1 || B > (int64_t)INT32_MAX / S || (ncols != 8 && ncols != 11)) return MVIP_EINVAL;
    if (B == 0) return MVIP_OK;
    if (!rows || !z || !weights || !loss) return MVIP_EINVAL;
    const dim3 grid((unsigned)((B + distortion::RAYS_PER_BLOCK - 1) / distortion::RAYS_PER_BLOCK)), block(distortion::BLOCK);
    if (lindisp)
        hipLaunchKernelGGL(distortion::distortion_loss_kernel<true>, grid, block, 0, as_stream(stream), rows, ncols, z, weights,
                           (long long)B, S, loss, grad);
    else
        hipLaunchKernelGGL(distortion::distortion_loss_kernel<false>, grid, block, 0, as_stream(stream), rows, ncols, z, weights,
                           (long long)B, S, loss, grad);
    return check_launch();
}
