// Pack the 24 state-dict tensors of the NeRF MLP into the streaming image (mlp_layout.h, mlp_image.h), and
// the inverse scatter for gradients.  2.4 MB each way, once per optimizer step: HBM-trivial.
#include "common.h"
#include "mlp_image.h"

namespace mvip {
using namespace mlp;

// float e of 1-KB block blk of the image -> (parameter tensor, element offset), or param = -1 for zero padding
__device__ __forceinline__ void packed_source(int blk, int e, int &param, int &off) {
    int lo;
    if (blk < TOTAL_BLOCKS) return image_source<Frag32>(blk, e, param, off, lo);
    param = -1; off = 0;
    const int j = (blk - TOTAL_BLOCKS) * BLOCK_FLOATS + e;
    if (j < SB_BFEAT) { param = 2 * (j / 256) + 1; off = j % 256; }
    else if (j < SB_BVIEWS) { param = P_BF; off = j - SB_BFEAT; }
    else if (j < SB_WALPHA) { param = P_BV; off = j - SB_BVIEWS; }
    else if (j < SB_BALPHA) { param = P_WA; off = j - SB_WALPHA; }
    else if (j == SB_BALPHA) { param = P_BA; off = 0; }
    else if (j >= SB_WRGB && j < SB_BRGB) { param = P_WR; off = j - SB_WRGB; }
    else if (j >= SB_BRGB && j < SB_BRGB + 3) { param = P_BR; off = j - SB_BRGB; }
}

// both kernels: one workgroup of BLOCK_FLOATS threads per 1-KB block of the image, sections A and B
constexpr int PACKED_BLOCKS = PACKED_FLOATS / BLOCK_FLOATS;
static_assert(PACKED_FLOATS % BLOCK_FLOATS == 0, "the image is whole blocks");

__global__ void mlp_pack_kernel(ParamPtrs pp, float *__restrict__ packed) {
    int param, off;
    packed_source(blockIdx.x, threadIdx.x, param, off);
    packed[blockIdx.x * BLOCK_FLOATS + threadIdx.x] = param >= 0 ? pp.p[param][off] : 0.f;
}

__global__ void mlp_unpack_grads_kernel(const float *__restrict__ gpacked, ParamPtrs gp, int accumulate) {
    int param, off;
    packed_source(blockIdx.x, threadIdx.x, param, off);
    if (param < 0) return;
    float *dst = const_cast<float *>(gp.p[param]) + off;      // the mapping is injective: no races
    const float g = gpacked[blockIdx.x * BLOCK_FLOATS + threadIdx.x];
    *dst = accumulate ? (*dst + g) : g;
}

}  // namespace mvip

using namespace mvip;

extern "C" int64_t mvip_mlp_packed_floats(void) { return mlp::PACKED_FLOATS; }

extern "C" int mvip_mlp_pack(const float *const *params_host, float *packed, void *stream) {
    mlp::ParamPtrs pp;
    if (!mlp::collect_params(params_host, pp) || !packed) return MVIP_EINVAL;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3(PACKED_BLOCKS), dim3(mlp::BLOCK_FLOATS), 0, as_stream(stream),
                       pp, packed);
    return check_launch();
}

extern "C" int mvip_mlp_unpack_grads(const float *grad_packed, float *const *grads_host, int accumulate,
                                     void *stream) {
    mlp::ParamPtrs gp;                                        // written through: the kernel casts the const away
    if (!mlp::collect_params(grads_host, gp) || !grad_packed) return MVIP_EINVAL;
    hipLaunchKernelGGL(mlp_unpack_grads_kernel, dim3(PACKED_BLOCKS), dim3(mlp::BLOCK_FLOATS), 0,
                       as_stream(stream), grad_packed, gp, accumulate);
    return check_launch();
}
