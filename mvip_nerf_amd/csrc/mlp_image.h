// The NeRF MLP as its weight images store it: ONE description of the stream's layers, of what W[row][k] of a layer is
// (padding included), of the transposed stream of the delta kernels, and the four fragment maps that are all the images
// differ in.  Every pack kernel is an instance of pack_image / pack_transposed below; the streaming kernels themselves
// only use the block offsets of mlp_layout.h.
#pragma once
#include <type_traits>
#include "common.h"
#include "mlp_layout.h"

namespace mvip { namespace mlp {

struct ParamPtrs { const float *p[P_COUNT]; };          // the 24 state-dict tensors (device pointers), by value to a kernel

// ---- the stream's layers --------------------------------------------------------------------------------------------
// One row per layer of section A, in stream order.  W[row][k], row < units, k < k_padded, is element
// row * k_real + (k - (k > zero_at)) of tensor `param`, and ZERO where k == zero_at or that column is >= k_real.
// zero_at is the one k where a zero is INSERTED between real columns (k_padded: the layer has none):
//   layer 0 reads 63 encoded inputs, then one zero; layer 5 reads [63 encoded | one zero | 256 hidden] from a 319-wide
//   tensor; the view layer reads 256 + 27 = 283 inputs, then 5 zeros.  This is the K padding rule of every image.
struct LayerRow { int first_block, units, k_padded, param, k_real, zero_at; };
constexpr int L_FEAT = 8, L_VIEWS = 9, N_STREAM_LAYERS = 10;
constexpr LayerRow LAYER[N_STREAM_LAYERS] = {
    {OFF_L0, 32 * L0_NT, 8 * L0_KG, P_W0, 63, 8 * L0_KG},
    {OFF_L1 + 0 * LH_BLOCKS, 256, 256, 2, 256, 256},
    {OFF_L1 + 1 * LH_BLOCKS, 256, 256, 4, 256, 256},
    {OFF_L1 + 2 * LH_BLOCKS, 256, 256, 6, 256, 256},
    {OFF_L1 + 3 * LH_BLOCKS, 256, 256, 8, 256, 256},
    {OFF_L5, 32 * L5_NT, 8 * L5_KG, 10, 319, 63},
    {OFF_L6 + 0 * LH_BLOCKS, 256, 256, 12, 256, 256},
    {OFF_L6 + 1 * LH_BLOCKS, 256, 256, 14, 256, 256},
    {OFF_FEAT, 256, 256, P_WF, 256, 256},
    {OFF_VIEWS, 32 * LV_NT, 8 * LV_KG, P_WV, 283, 8 * LV_KG},
};
static_assert(LAYER[L_VIEWS].first_block * BLOCK_FLOATS + LAYER[L_VIEWS].units * LAYER[L_VIEWS].k_padded == SEC_A_FLOATS,
              "the table covers section A");

// Both lookups are compare chains over the constexpr table (fully unrolled: selects of immediates, no memory table; the
// pack kernels call them with a workgroup-uniform argument, so they are scalar instructions).
__host__ __device__ inline LayerRow layer_row(int layer) {
    LayerRow r = LAYER[0];
#pragma unroll
    for (int i = 1; i < N_STREAM_LAYERS; ++i) if (layer == i) r = LAYER[i];
    return r;
}
// the layer that stream block `blk` belongs to, and the block's index inside it
__host__ __device__ inline LayerRow layer_of_block(int blk, int &local) {
    LayerRow r = LAYER[0];
#pragma unroll
    for (int i = 1; i < N_STREAM_LAYERS; ++i) if (blk >= LAYER[i].first_block) r = LAYER[i];
    local = blk - r.first_block;
    return r;
}

// W[row][k] of a layer -> (parameter tensor, element offset); param = -1 where the image holds a padding zero
__host__ __device__ inline void weight_source(const LayerRow &L, int row, int k, int &param, int &off) {
    const int col = k - (k > L.zero_at);
    const bool real = k != L.zero_at && col < L.k_real;
    param = real ? L.param : -1;
    off = real ? row * L.k_real + col : 0;
}
__device__ __forceinline__ float weight_at(const ParamPtrs &pp, const LayerRow &L, int row, int k) {
    int param, off;
    weight_source(L, row, k, param, off);
    return param >= 0 ? pp.p[param][off] : 0.f;
}

// ---- the transposed stream (delta kernels) --------------------------------------------------------------------------
// W^T of: the view layer (its 256 feature inputs only), feature, then layers 7, 6, 5 (its h4 part: k = 64 + in), 4, 3, 2, 1.
// Transposed layer m has 256 rows (input units of the forward layer) and K = the forward layer's `units`.  The block
// counts are the same in every format (a block is 1 KB in each).
constexpr int T_VIEWS_BLOCKS = 256 * 128 / BLOCK_FLOATS;                 // 128
constexpr int T_LAYER_BLOCKS = 256 * 256 / BLOCK_FLOATS;                 // 256
constexpr int T_TOTAL_BLOCKS = T_VIEWS_BLOCKS + 8 * T_LAYER_BLOCKS;      // 2176
constexpr int T_TOTAL_CHUNKS = T_TOTAL_BLOCKS / CHUNK_BLOCKS;            // 136
constexpr int T_FLOATS = T_TOTAL_BLOCKS * BLOCK_FLOATS;
static_assert(T_TOTAL_BLOCKS % CHUNK_BLOCKS == 0, "the transposed stream is whole chunks");

// transposed layer m = 0..8 -> the forward layer it transposes and the first of that layer's k it covers
__host__ __device__ inline LayerRow transposed_source(int m, int &k0) {
    const int layer = m == 0 ? L_VIEWS : m == 1 ? L_FEAT : 9 - m;
    k0 = layer == 5 ? 64 : 0;
    return layer_row(layer);
}
__host__ __device__ inline int transposed_layer_of_block(int blk, int &local) {
    const int m = blk < T_VIEWS_BLOCKS ? 0 : 1 + (blk - T_VIEWS_BLOCKS) / T_LAYER_BLOCKS;
    local = m == 0 ? blk : (blk - T_VIEWS_BLOCKS) % T_LAYER_BLOCKS;
    return m;
}

// ---- the four fragment formats ----------------------------------------------------------------------------------------
// A format says where in a layer's blocks the element for output row `row` and input unit `k` sits:
//   decode(local block, element of the block, K of the layer) -> (row, k, lo);   index(row, k, K) -> element of the layer
// (inverse of decode for lo = 0; in the fp16 formats the lo term sits BLOCK_ELEMS further on: [Ah | Al] per k-step).

// fp32, 32 points per wave (v_mfma_f32_32x32x2_f32; mlp_fwd.hip, mlp_delta_kernel).  Lane (i = lane & 31, h = lane >> 5) of
// block (tile ti, k-group kg) holds W[32 ti + i][8 kg + 4 h + s], s = 0..3, at float h * 128 + i * 4 + s (mlp_layout.h says
// why).  Output tiles are consumed in PAIRS: the blocks of tiles (2P, 2P + 1) alternate, k-group by k-group.
struct Frag32 {
    using elem = float;
    static constexpr int BLOCK_ELEMS = 256;
    // position of block (tile ti, k-group kg) inside a layer with KG k-groups per tile, and its inverse
    __host__ __device__ static constexpr int block_pos(int ti, int kg, int KG) { return (ti >> 1) * (2 * KG) + 2 * kg + (ti & 1); }
    __host__ __device__ static void block_tile(int local, int KG, int &ti, int &kg) {
        // pair = local / (2 KG): a layer has at most 8 tiles = 4 pairs, so three compares stand in for a division by a
        // variable.  Forward layers: the assert; transposed layers: 256 rows each (transposed_source), 8 tiles as well.
        static_assert(L0_NT <= 8 && LH_NT <= 8 && L5_NT <= 8 && LV_NT <= 8, "at most 4 tile pairs per layer");
        const int pair = (local >= 2 * KG) + (local >= 4 * KG) + (local >= 6 * KG), rem = local - pair * 2 * KG;
        kg = rem >> 1;
        ti = 2 * pair + (rem & 1);
    }
    __host__ __device__ static void decode(int local, int e, int K, int &row, int &k, int &lo) {
        int ti, kg;
        block_tile(local, K / 8, ti, kg);
        const int h = e / 128, i = (e % 128) / 4, s = e % 4;
        row = 32 * ti + i; k = 8 * kg + 4 * h + s; lo = 0;
    }
    __host__ __device__ static int index(int row, int k, int K) {
        return block_pos(row >> 5, k >> 3, K / 8) * BLOCK_ELEMS + ((k & 7) >> 2) * 128 + (row & 31) * 4 + (k & 3);
    }
};

// fp32, 16 points per wave (v_mfma_f32_16x16x4_f32; mlp_fwd16_kernel.h, mlp_delta16_kernel).  Block (out tile `to`, in tile
// ti), output tile by output tile: lane (m = lane & 15, g = lane >> 4) holds W[16 to + m][16 ti + 4 g + 0..3], four
// consecutive input units -- one ds_read_b128 feeds four MFMAs.
struct Frag16 {
    using elem = float;
    static constexpr int BLOCK_ELEMS = 256;
    __host__ __device__ static void decode(int local, int e, int K, int &row, int &k, int &lo) {
        const int nti = K / 16, lane = e / 4;
        row = 16 * (local / nti) + (lane & 15); k = 16 * (local % nti) + 4 * (lane >> 4) + e % 4; lo = 0;
    }
    __host__ __device__ static int index(int row, int k, int K) {
        return ((row >> 4) * (K / 16) + (k >> 4)) * BLOCK_ELEMS + (((k & 15) >> 2) * 16 + (row & 15)) * 4 + (k & 3);
    }
};

// fp16 hi | lo, 32 points per wave (v_mfma_f32_32x32x16_f16; mlp_fwd_f16x3.hip, mlp_delta_f16x3_kernel).  Blocks (tile ti,
// k-step ks, hi | lo), tile by tile: element j of lane (i = lane & 31, h = lane >> 5) is W[32 ti + i][16 ks + 8 (j >> 2) +
// 4 h + (j & 3)] -- the k order in which a 32x32 accumulator tile's registers form the next layer's B operand.
struct FragH32 {
    using elem = _Float16;
    static constexpr int BLOCK_ELEMS = 512;
    __host__ __device__ static void decode(int local, int e, int K, int &row, int &k, int &lo) {
        const int ksn = K / 16, pair = local / 2, lane = e / 8, j = e % 8;
        row = 32 * (pair / ksn) + lane % 32; k = 16 * (pair % ksn) + 8 * (j >> 2) + 4 * (lane / 32) + (j & 3); lo = local % 2;
    }
    __host__ __device__ static int index(int row, int k, int K) {
        const int r = k & 15, j = ((r >> 3) << 2) | (r & 3), h = (r & 7) >> 2;
        return 2 * ((row >> 5) * (K / 16) + (k >> 4)) * BLOCK_ELEMS + (h * 32 + (row & 31)) * 8 + j;
    }
};

// fp16 hi | lo, 16 points per wave (v_mfma_f32_16x16x32_f16; mlp_fwd16_f16x3.hip).  Blocks (tile `to`, k-step s, hi | lo):
// element j of lane (m = lane & 15, g = lane >> 4) is W[16 to + m][32 s + unit_of(g, j)]: k-slot (g, j) of a K = 32 step is
// register j of 16-unit tile 2s (j < 4) or 2s + 1 (j >= 4) of lane group g.
struct FragH16 {
    using elem = _Float16;
    static constexpr int BLOCK_ELEMS = 512;
    __host__ __device__ static constexpr int unit_of(int g, int j) { return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4); }
    __host__ __device__ static void decode(int local, int e, int K, int &row, int &k, int &lo) {
        const int ksn = K / 32, pair = local / 2, lane = e / 8;
        row = 16 * (pair / ksn) + (lane & 15); k = 32 * (pair % ksn) + unit_of(lane >> 4, e % 8); lo = local % 2;
    }
    __host__ __device__ static int index(int row, int k, int K) {
        const int u = k & 31, g = (u & 15) >> 2, j = 4 * (u >> 4) + (u & 3);
        return 2 * ((row >> 4) * (K / 32) + (k >> 5)) * BLOCK_ELEMS + (g * 16 + (row & 15)) * 8 + j;
    }
};

// what an image element holds of weight w: w itself, or one term of the fp16 split  hi = f16(w), lo = f16(w - hi)
template <class T>
__device__ __forceinline__ T image_value(float w, int lo) {
    if constexpr (std::is_same<T, float>::value) return w;
    else { const _Float16 wh = (_Float16)w; return lo ? (_Float16)(w - (float)wh) : wh; }
}
// and back: element e of a layer as fp32 (hi + lo is exact in fp32)
template <class F>
__device__ __forceinline__ float image_load(const typename F::elem *__restrict__ layer, int e) {
    if constexpr (std::is_same<typename F::elem, float>::value) return layer[e];
    else return (float)layer[e] + (float)layer[e + F::BLOCK_ELEMS];
}

// ---- pack kernel bodies -----------------------------------------------------------------------------------------------
// A workgroup of PACK_THREADS threads handles consecutive elements of ONE block, so the block index comes from blockIdx
// alone and everything that depends only on the block -- which layer, which tile -- is scalar work, once per wave.
constexpr int PACK_THREADS = 256;
template <class F> constexpr unsigned pack_image_grid() { return TOTAL_BLOCKS * (F::BLOCK_ELEMS / PACK_THREADS); }
template <class F> constexpr unsigned pack_transposed_grid() { return T_TOTAL_BLOCKS * (F::BLOCK_ELEMS / PACK_THREADS); }
template <class F>
__device__ __forceinline__ void workgroup_element(int &blk, int &e) {
    static_assert(F::BLOCK_ELEMS % PACK_THREADS == 0, "a workgroup stays inside one block");
    constexpr int PER_BLOCK = F::BLOCK_ELEMS / PACK_THREADS;
    blk = blockIdx.x / PER_BLOCK;
    e = (blockIdx.x % PER_BLOCK) * PACK_THREADS + threadIdx.x;
}

// element e of section-A block blk in format F -> (parameter tensor or -1, offset, lo term)
template <class F>
__host__ __device__ inline void image_source(int blk, int e, int &param, int &off, int &lo) {
    int local, row, k;
    const LayerRow L = layer_of_block(blk, local);
    F::decode(local, e, L.k_padded, row, k, lo);
    weight_source(L, row, k, param, off);
}
template <class F>
__device__ __forceinline__ void pack_image(const ParamPtrs &pp, typename F::elem *__restrict__ img) {
    int blk, e, param, off, lo;
    workgroup_element<F>(blk, e);
    image_source<F>(blk, e, param, off, lo);
    img[blk * F::BLOCK_ELEMS + e] = image_value<typename F::elem>(param >= 0 ? pp.p[param][off] : 0.f, lo);
}
// the transposed stream in format Dst from the forward image in format Src (same element type)
template <class Dst, class Src>
__device__ __forceinline__ void pack_transposed(const typename Src::elem *__restrict__ img, typename Dst::elem *__restrict__ out) {
    int blk, e, local, k0, in, o, lo;
    workgroup_element<Dst>(blk, e);
    const LayerRow L = transposed_source(transposed_layer_of_block(blk, local), k0);
    Dst::decode(local, e, L.units, in, o, lo);                          // row of W^T = input unit, column = output unit
    const float w = image_load<Src>(img + L.first_block * Src::BLOCK_ELEMS, Src::index(o, k0 + in, L.k_padded));
    out[blk * Dst::BLOCK_ELEMS + e] = image_value<typename Dst::elem>(w, lo);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// the 24 device pointers of a host array, all non-null
static inline bool collect_params(const float *const *params_host, ParamPtrs &pp) {
    if (!params_host) return false;
    for (int i = 0; i < P_COUNT; ++i) {
        if (!params_host[i]) return false;
        pp.p[i] = params_host[i];
    }
    return true;
}
// section B (fp32 biases / head rows) of every image is the fp32 image's; call after the section-A launch
static inline int finish_with_section_b(float *image, const float *packed_f32, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(image + SEC_A_FLOATS, packed_f32 + SEC_A_FLOATS, sizeof(float) * SEC_B_FLOATS,
                                        hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { set_last_error(e); return MVIP_ELAUNCH; }
    return check_launch();
}

}}  // namespace mvip::mlp
