// Test probe of the 16-point kernels' input encoding (mlp_device16.h): the per-channel route (enc_channel, one sinf or cosf
// per fragment channel and lane -- what the kernels ran before encode16_wave, kept here only as the reference) and the
// once-per-wave route (encode16_wave), side by side on the same points.  Same workgroup shape and lane roles as the real
// kernels: 512 threads = 8 waves of 16 points, lane (n, g) holds channels 16 t + 4 g .. + 3 of point n.
#include "mlp_device16.h"

namespace mvip {
namespace f16p {

__global__ void __launch_bounds__(512) mlp_encode16_probe_kernel(const float *__restrict__ pts, const float *__restrict__ dirs,
                                                                  int64_t P, float *__restrict__ out_old,
                                                                  float *__restrict__ out_new) {
    __shared__ __attribute__((aligned(16))) float stage[8 * ENC_STAGE_FLOATS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 15, g = lane >> 4;
    int64_t p = (int64_t)blockIdx.x * WG_POINTS + wave * 16 + n;
    const bool live = p < P;
    if (!live) p = P - 1;
    const float px = pts[p * 3], py = pts[p * 3 + 1], pz = pts[p * 3 + 2];
    const float vx = dirs[p * 3], vy = dirs[p * 3 + 1], vz = dirs[p * 3 + 2];

    f32x4 emb[4], edir[2];
    encode16_wave(stage + wave * ENC_STAGE_FLOATS, lane, px, py, pz, vx, vy, vz, emb, edir);
    f32x4 emb0[4], edir0[2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) emb0[t][i] = enc_channel<63>(px, py, pz, 16 * t + 4 * g + i);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) edir0[t][i] = enc_channel<27>(vx, vy, vz, 16 * t + 4 * g + i);
    if (!live) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        *reinterpret_cast<f32x4 *>(out_new + p * 96 + 16 * t + 4 * g) = emb[t];
        *reinterpret_cast<f32x4 *>(out_old + p * 96 + 16 * t + 4 * g) = emb0[t];
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        *reinterpret_cast<f32x4 *>(out_new + p * 96 + 64 + 16 * t + 4 * g) = edir[t];
        *reinterpret_cast<f32x4 *>(out_old + p * 96 + 64 + 16 * t + 4 * g) = edir0[t];
    }
}

}  // namespace f16p
}  // namespace mvip

using namespace mvip;
using namespace mvip::f16p;

// pts, dirs [P,3] -> out_old, out_new [P,96] fp32: the 64 position channels (63 + a zero) then the 32 direction channels
// (27 + 5 zeros), in Embedder order.
extern "C" int mvip_mlp_encode16_probe(const float *pts, const float *dirs, int64_t P, float *out_old, float *out_new,
                                       void *stream) {
    if (P < 0) return MVIP_EINVAL;
    if (P == 0) return MVIP_OK;
    if (!pts || !dirs || !out_old || !out_new) return MVIP_EINVAL;
    hipLaunchKernelGGL(mlp_encode16_probe_kernel, dim3((unsigned)((P + WG_POINTS - 1) / WG_POINTS)), dim3(512), 0,
                       as_stream(stream), pts, dirs, P, out_old, out_new);
    return check_launch();
}
