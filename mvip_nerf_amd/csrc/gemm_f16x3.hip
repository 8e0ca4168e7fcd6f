// The plain GEMM of the SDS networks in split precision ("f16x3", operand format and scale rule: csrc/f16x3_operand.h) -- the
// 1x1 convolutions and linear layers of the UNet's transformer blocks, the attention projections, and the strided /
// narrow-channel convolutions that run as im2col + GEMM.  A (weights) is packed once per layer by gm_pack_kernel, X
// (activations) arrives in the split planes the producers of csrc/f16x3_producers.hip and the operand sinks
// (csrc/plane_sink.h) write.  Three kernels: operands through LDS (gemm_f16x3_kernel), B streamed into registers
// (gemm5_f16x3_kernel, the default) and a square-ish workgroup tile (gemm2_f16x3_kernel).
#include "f16x3_operand.h"
#include "plane_sink.h"
#include <stdlib.h>

namespace mvip {

// A operand of the plain GEMM (1x1 "convolution"): A[m][k] = src[m*sm + k*sk], packed [M/32][K/16][hl][lane][8]
__global__ void gm_pack_kernel(const float *__restrict__ src, int M, int K, int64_t sm, int64_t sk,
                               const float *__restrict__ scale2, uint4 *__restrict__ out, unsigned *__restrict__ lo_flag) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int CK = K / 16;
    const int64_t total = (int64_t)(M / 32) * CK * 2 * 64;
    if (idx >= total) return;
    int64_t r = idx;
    const int lane = (int)(r % 64); r /= 64;
    const int hl = (int)(r % 2); r /= 2;
    const int ck = (int)(r % CK); r /= CK;
    const int m = (int)r * 32 + (lane & 31);
    const int kg = lane >> 5;
    const float s = scale2[0];
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)m * sm + (int64_t)(ck * 16 + kg * 8 + j) * sk] * s;
    uint4 hi, lo;
    split8(v, hi, lo);
    out[idx] = hl ? lo : hi;
    if (hl) note_lo(lo, lo_flag);
}

// The reduction of a split-K launch (cv_split_reduce_kernel, csrc/conv3x3.hip) whose result leaves as split planes
// [N][M/16][2][2][P][8 halves] * out_scale (an operand sink behind a split-K launch): thread = (sample, 8-row block, column);
// the 8 rows of a fragment are 8 coalesced row reads per split.
__global__ void __launch_bounds__(256)
cv_split_reduce_planes_kernel(const float *__restrict__ partial, int splits, int N, int M, int64_t P,
                              const float *__restrict__ w_scale2, const float *__restrict__ x_scale2,
                              const float *__restrict__ bias, const float *__restrict__ residual, float out_scale,
                              uint4 *__restrict__ planes, int prec) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int blk = blockIdx.y % (M / 8), n = blockIdx.y / (M / 8);
    if (p >= P) return;
    const float inv = w_scale2[1] * (x_scale2 ? x_scale2[1] : 1.f);
    const int64_t total = (int64_t)N * M * P;
    const int64_t base = ((int64_t)n * M + blk * 8) * P + p;
    float sum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = partial[base + j * P];
    for (int s = 1; s < splits; ++s) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = partial[(int64_t)s * total + base + j * P];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[j] += t[j];
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float t = sum[j] * inv;
        if (bias) t += bias[blk * 8 + j];
        if (residual) t += residual[base + j * P];
        v[j] = t * out_scale;
    }
    uint4 hi, lo;
    split8(v, hi, lo);
    uint4 *dst = planes + (((int64_t)n * (M / 16) + (blk >> 1)) * 4 + (blk & 1) * 2) * P + p;
    dst[0] = hi;
    if (prec != 1) dst[P] = lo;
}

// ---- plain GEMM (1x1 convolution, attention products) on the same operand formats -----------------------
//   Y[n][m][p] = sum_k A[m][k] X[n][k][p] / (s_a s_x) + bias[m] + chan_add[n][m] + residual[n][m][p]
// A packed by gm_pack_kernel, X in split planes [n][K/16][2][2][P][8].  Workgroup = 32*MT rows x 256
// columns, stage = 32 k (two 16-channel chunks: 48 MFMAs per wave at MT=4), double-buffered DMA.
constexpr int GM_PIX = 256;
constexpr int GM_KC = 2;
constexpr int64_t GM_P_MAX = (int64_t)1 << 26;      // columns per sample: the streamed kernel's per-lane 32-bit plane offsets

struct GemmArgs {
    const char *xs, *wp;
    const float *bias, *chan_add, *residual, *x_scale2, *w_scale2;
    float *y;
    int N, CK, M, MB, tiles;
    int64_t P;
    // GEGLU epilogue (MT = 2 only): the rows are interleaved in 32-row tiles (value tile, gate tile); the kernel
    // writes value * gelu(gate) as [N][M/2][P], zero for columns >= geglu_L, and collects the absolute maximum
    int geglu_L;                 // 0: plain epilogue
    unsigned *absmax_bits;
    // split-K (gemm_f16x3_kernel only; partial != nullptr): workgroup `split` contracts stages [split*sks, (split+1)*sks)
    // and writes raw accumulators to partial[split][n][M][P]; cv_split_reduce_kernel adds them in order
    int splits, sks;
    float *partial;
    // Operand sinks (nsec > 0; gemm5_f16x3_kernel only): the M rows are cut into <= 3 consecutive sections (multiples of
    // 64 rows), each written in the operand format of the contraction that consumes it, scaled by a power of two fixed
    // before the launch: kind 1 = split planes [N][rows/16][2][2][P][8] (also the GEGLU product when geglu_L > 0, rows =
    // M/2), kind 2 = attention V fragments [N][heads][DT][P/16][2][64][8] -- that section is computed TRANSPOSED (the MFMA
    // operands swapped: lane = output row, registers = tokens), which is the fragment order of csrc/attention.hip.
    // y is not written for these rows.
    struct Sec { char *ptr; float scale; int row_end, kind; } sec[3];
    int nsec, v_dt;              // v_dt: 32-row tiles per head in a kind-2 section
    int prec;                    // 1: single fp16 product (hi planes / hi fragments only; sinks write no lo halves)
    // LayerNorm statistics of the OUTPUT (plain fp32 epilogue, unsplit launches only): the rows are the channels a later
    // LayerNorm reduces over, so each workgroup leaves, per column (token), the fp64 sum and sum of squares of its 32 MT
    // finished rows in the layout ln_stats_kernel (csrc/transformer.hip) writes for 64-channel segments:
    // ln_part[((n * MB + mb) * 2 + {0, 1}) * P + p].  The statistics launch of the next LayerNorm disappears.
    double *ln_part;
#ifdef MVIP_EXPERIMENT_GEMM
    int dbg;                     // timing experiments: 1 = no epilogue stores, 2 = no MFMAs, 4 = no LDS reads either
#endif
};

// epilogue of the SWAP instantiation: the accumulators are transposed (lane = row of the weight tile, registers = the 32
// tokens of column block j) and leave as attention V fragments [N][heads][v_dt][P/16][2][64][8 halves]; the launch's M
// rows are the heads * v_dt * 32 rows of ONE section (a.sec[0])
template <int MT>
__device__ __forceinline__ void gemm_epilogue_vfrag(const GemmArgs &a, f32x16 (&acc)[MT][2], int n, int mb, int64_t p0, int wave,
                                                    int lane) {
    const int l32 = lane & 31;
    const float sc = a.sec[0].scale;
    const float mul = a.w_scale2[1] * (a.x_scale2 ? a.x_scale2[1] : 1.f) * sc;
    const bool hb = a.bias != nullptr;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int lt = mb * MT + m;                            // (head, dt) block of this row tile: lt = head * v_dt + dt
        const float bs = hb ? a.bias[lt * 32 + l32] * sc : 0.f;
        char *vt = a.sec[0].ptr + ((int64_t)n * (a.M / 32) + lt) * (a.P / 16) * 2048;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = acc[m][j][r] * mul + bs;
            sink_store_vfrag(vt, (int)((p0 + (2 * wave + j) * 32) / 16), lane, v, a.prec != 1);
        }
    }
}

// epilogue shared by the 32/64-row GEMM kernels: acc[m][j] = 32 x 32 tile (row tile mb*MT + m, columns p0 + (2 wave + j)*32 ..)
// LN: the instantiation can leave LayerNorm statistics (GemmArgs::ln_part; the B-in-registers kernel only -- in the
// LDS-staged kernel the extra live registers spilled)
template <int MT, bool LN = false>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs &a, f32x16 (&acc)[MT][2], int n, int mb, int64_t p0, int split,
                                              int wave, int lane) {
    const int l32 = lane & 31, kg = lane >> 5;
    const float inv = a.w_scale2[1] * (a.x_scale2 ? a.x_scale2[1] : 1.f);
#ifdef MVIP_EXPERIMENT_GEMM
    if (a.dbg & 1) {
        float t = 0.f;
        for (int m = 0; m < MT; ++m) for (int j = 0; j < 2; ++j) for (int r = 0; r < 16; ++r) t += acc[m][j][r];
        if (t == 123.456f) a.y[0] = t;
        return;
    }
#endif
    // all loads of the epilogue are issued together, ahead of the arithmetic (see the convolution's epilogue)
    const bool hb = a.bias != nullptr, hc = a.chan_add != nullptr, hr = a.residual != nullptr;
    if (a.nsec > 0 && a.geglu_L == 0 && !a.partial) {       // (split-K: raw partial sums first, the sink is the reduce launch)
        // ---- operand sinks: this workgroup's MT row tiles lie in ONE section (sections are multiples of 64 rows) ----
        const int row0 = mb * MT * 32;
        GemmArgs::Sec sc = a.sec[0];                 // static indices only: a dynamically indexed kernel argument goes to scratch
        int sec_row0 = 0;
        if (a.nsec > 1 && row0 >= a.sec[0].row_end) { sc = a.sec[1]; sec_row0 = a.sec[0].row_end; }
        if (a.nsec > 2 && row0 >= a.sec[1].row_end) { sc = a.sec[2]; sec_row0 = a.sec[1].row_end; }
        {
            const int n_blk8 = (sc.row_end - sec_row0) / 8;
            char *pn = sc.ptr + (int64_t)n * (n_blk8 / 2) * 4 * a.P * 16;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float bv[16];
                f32x16 rv[2];
                if (hr) {                                       // the residual stream joins before the split (loads issued together)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            rv[j][r] = a.residual[((int64_t)n * a.M + row0 + m * 32 + 8 * (r >> 2) + 4 * kg + (r & 3)) * a.P + p0 +
                                                  (2 * wave + j) * 32 + l32];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = hb ? a.bias[row0 + m * 32 + 8 * (r >> 2) + 4 * kg + (r & 3)] : 0.f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float v[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float t = acc[m][j][r] * inv;           // the fp32 epilogue's order of roundings, then the scale
                        if (hb) t += bv[r];
                        if (hr) t += rv[j][r];
                        v[r] = t * sc.scale;
                    }
                    sink_store_planes(pn, a.P, (row0 - sec_row0) / 8 + m * 4, n_blk8, p0 + (2 * wave + j) * 32 + l32, kg, v, true, a.prec != 1);
                }
            }
        }
        return;
    }
    if (MT == 2 && a.geglu_L > 0) {
        // feed-forward first projection: out = value * gelu(gate) (erf form), the two halves sit in this workgroup's
        // two row tiles; the [N][8C][P] intermediate never exists
        float ba[16], bg[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int r32 = 8 * (r >> 2) + 4 * kg + (r & 3);
            ba[r] = hb ? a.bias[(mb * 2 + 0) * 32 + r32] : 0.f;
            bg[r] = hb ? a.bias[(mb * 2 + 1) * 32 + r32] : 0.f;
        }
        if (a.nsec > 0) {
            // the product goes out as the second projection's operand planes, scaled by a power of two fixed before the
            // launch (|value * gelu(gate)| <= |value| |gate|): no absolute-maximum collection, no fp32 intermediate
            const int n_blk8 = (a.M / 2) / 8;
            char *pn = a.sec[0].ptr + (int64_t)n * (n_blk8 / 2) * 4 * a.P * 16;
            const float os = a.sec[0].scale;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t px = p0 + (2 * wave + j) * 32 + l32;
                float v[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float av = acc[0][j][r] * inv, gv = acc[MT - 1][j][r] * inv;
                    if (hb) { av += ba[r]; gv += bg[r]; }
                    const float t = av * (0.5f * gv * (1.0f + erff(gv * 0.70710678118654752f)));
                    v[r] = px >= a.geglu_L ? 0.f : t * os;
                }
                sink_store_planes(pn, a.P, mb * 4, n_blk8, px, kg, v, true, a.prec != 1);
            }
            return;
        }
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t px = p0 + (2 * wave + j) * 32 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int r32 = 8 * (r >> 2) + 4 * kg + (r & 3);
                float av = acc[0][j][r] * inv, gv = acc[MT - 1][j][r] * inv;
                if (hb) { av += ba[r]; gv += bg[r]; }
                float v = av * (0.5f * gv * (1.0f + erff(gv * 0.70710678118654752f)));
                if (px >= a.geglu_L) v = 0.f;
                mx = absmax_take(mx, v);
                a.y[((int64_t)n * (a.M / 2) + mb * 32 + r32) * a.P + px] = v;
            }
        }
        mx = wave_max(mx);
        if (lane == 0) atomicMax(a.absmax_bits, __float_as_uint(mx));
        return;
    }
    auto out_index = [&](int m, int j, int r, int &row) -> int64_t {
        row = (mb * MT + m) * 32 + 8 * (r >> 2) + 4 * kg + (r & 3);
        return ((int64_t)n * a.M + row) * a.P + p0 + (2 * wave + j) * 32 + l32;
    };
    if (a.partial) {
        float *pp = a.partial + (int64_t)split * a.N * a.M * a.P;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { int row; pp[out_index(m, j, r, row)] = acc[m][j][r]; }
        return;
    }
    float bv[MT][16], cv[MT][16];
    f32x16 rv[MT][2];
    if (hr) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { int row; rv[m][j][r] = a.residual[out_index(m, j, r, row)]; }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (mb * MT + m) * 32 + 8 * (r >> 2) + 4 * kg + (r & 3);
            bv[m][r] = hb ? a.bias[row] : 0.f;
            cv[m][r] = hc ? a.chan_add[(int64_t)n * a.M + row] : 0.f;
        }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row;
                const int64_t o = out_index(m, j, r, row);
                float v = acc[m][j][r] * inv;
                if (hb) v += bv[m][r];
                if (hc) v += cv[m][r];
                if (hr) v += rv[m][j][r];
                a.y[o] = v;
                if constexpr (LN) acc[m][j][r] = v;             // kept for the statistics below
            }
    if constexpr (LN) if (a.ln_part) {
        // a lane holds 16 MT rows of each of its two columns; the other half-wave (kg) holds the other 16 MT rows of the
        // same columns: in-register fp64 sums + one cross-half add, no LDS
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double sm = 0.0, q = 0.0;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) { const double t = (double)acc[m][j][r]; sm += t; q += t * t; }
            sm += __shfl_xor(sm, 32, 64);
            q += __shfl_xor(q, 32, 64);
            if (kg == 0) {
                const int64_t p = p0 + (2 * wave + j) * 32 + l32;
                double *dst = a.ln_part + (((int64_t)n * a.MB + mb) * 2) * a.P + p;
                dst[0] = sm;
                dst[a.P] = q;
            }
        }
    }
}

template <int MT>
__global__ void __launch_bounds__(256, (MT <= 2 ? 2 : 1)) gemm_f16x3_kernel(const GemmArgs a) {
    constexpr int WB = GM_KC * MT * 2 * 1024;
    constexpr int IB = GM_KC * 4 * GM_PIX * 16;
    __shared__ __attribute__((aligned(16))) char lds[2 * WB + 2 * IB];
    char *lds_w = lds, *lds_in = lds + 2 * WB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, kg = lane >> 5;
    int id = blockIdx.x;
    const int total = gridDim.x;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    const int split = id % a.splits;
    id /= a.splits;
    const int mb = id % a.MB;
    const int tile = id / a.MB;
    const int tp = tile % a.tiles;
    const int n = tile / a.tiles;
    const int64_t p0 = (int64_t)tp * GM_PIX;
    const int64_t plane = a.P * 16;
    const int s0 = split * a.sks;                       // first stage (of GM_KC chunks) of this workgroup
    const char *xs_n = a.xs + ((int64_t)n * a.CK + s0 * GM_KC) * 4 * plane + (p0 + tid) * 16;

    auto issue_input = [&](int s, int buf) {
#pragma unroll
        for (int kc = 0; kc < GM_KC; ++kc)
#pragma unroll
            for (int piece = 0; piece < 4; ++piece)
                glds16b(xs_n + ((int64_t)(s * GM_KC + kc) * 4 + piece) * plane,
                        lds_in + buf * IB + ((kc * 4 + piece) * GM_PIX + wave * 64) * 16);
    };
    auto issue_weights = [&](int s, int buf) {
#pragma unroll
        for (int b0 = 0; b0 < GM_KC * MT * 2; b0 += 4) {       // LDS block b = (kc*MT + m)*2 + hl
            const int b = b0 + wave;
            if (b < GM_KC * MT * 2) {
                const int hl = b & 1, m = (b >> 1) % MT, kc = (b >> 1) / MT;
                glds16b(a.wp + ((((int64_t)(mb * MT + m) * a.CK + (s0 + s) * GM_KC + kc) * 2 + hl) * 1024) + lane * 16,
                        lds_w + buf * WB + b * 1024);
            }
        }
    };

    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

    const int nall = a.CK / GM_KC;
    const int nstage = (nall - s0 < a.sks) ? nall - s0 : a.sks;
    issue_input(0, 0);
    issue_weights(0, 0);
    for (int s = 0; s < nstage; ++s) {
        __syncthreads();
        if (s + 1 < nstage) { issue_weights(s + 1, (s + 1) & 1); issue_input(s + 1, (s + 1) & 1); }
        const char *inb = lds_in + (s & 1) * IB;
        const char *wb = lds_w + (s & 1) * WB + lane * 16;
#pragma unroll
        for (int kc = 0; kc < GM_KC; ++kc) {
            h16x8 bh[2], bl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int p = (2 * wave + j) * 32 + l32;
                bh[j] = *reinterpret_cast<const h16x8 *>(inb + ((kc * 4 + kg * 2 + 0) * GM_PIX + p) * 16);
                bl[j] = *reinterpret_cast<const h16x8 *>(inb + ((kc * 4 + kg * 2 + 1) * GM_PIX + p) * 16);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const h16x8 ah = *reinterpret_cast<const h16x8 *>(wb + ((kc * MT + m) * 2 + 0) * 1024);
                const h16x8 al = *reinterpret_cast<const h16x8 *>(wb + ((kc * MT + m) * 2 + 1) * 1024);
#ifdef MVIP_EXPERIMENT_GEMM
                if (a.dbg & 2) { acc[m][0][0] += (float)ah[0] + (float)bh[0][0] + (float)bl[1][0] + (float)al[0] + (float)bh[1][0] + (float)bl[0][0]; continue; }
#endif
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[j], acc[m][j], 0, 0, 0);
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[j], acc[m][j], 0, 0, 0);
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[j], acc[m][j], 0, 0, 0);
                }
            }
        }
    }
    gemm_epilogue<MT>(a, acc, n, mb, p0, split, wave, lane);
}

// ---- the same GEMM with the B operand streamed straight into registers ----------------------------------------------
// The kernel above is bound by operand delivery: 36 KB of DMA per 12 MFMAs and workgroup (94 B/clk/CU at the matrix rate)
// with ONE stage in flight, where L2 -> CU delivery needs ~64 KB in flight per CU to reach its ~57 B/clk
// (tools/micro/l2_load_bw.hip) -- PMC: matrix pipe 12 % busy, 54 % of the wave time in s_waitcnt.  Here
//  * the B operand (activations: no reuse between the four waves, each owns 64 columns) never touches LDS: a lane's
//    fragment is 16 contiguous bytes of a split plane, so the MFMA operand registers are loaded directly
//    (global_load_dwordx4, 512 B contiguous per half-wave), SIX 16-k chunks (24 loads, 24 KB per wave) ahead of their use;
//  * the A operand (weights, shared by the four waves) streams through a three-slot LDS ring of 64-k chunks by LDS-DMA,
//    two chunks ahead; the only synchronisation is one s_barrier per chunk WITHOUT a vmcnt(0) drain: loads return in
//    order, and the wave has by then waited for B fragments that were issued after the chunk's DMA (DB <= 7), so its
//    share of that DMA has landed.
// Same grid, operand formats, split-K and epilogue as gemm_f16x3_kernel.
template <int V> struct cic { static constexpr int value = V; };
template <int N, class F, int I = 0>
__device__ __forceinline__ void cv_static_for(F &&f) {
    if constexpr (I < N) { f(cic<I>{}); cv_static_for<N, F, I + 1>(static_cast<F &&>(f)); }
}
constexpr int G5_DB = 6;        // B prefetch depth in 16-k chunks
constexpr int G5_CA = 4;        // 16-k chunks per A ring slot
template <int MT, bool SWAP = false, int NP = 3>
__global__ void __launch_bounds__(256, MT == 1 ? 3 : 2) gemm5_f16x3_kernel(const GemmArgs a) {
    constexpr bool F16 = NP == 1;
    constexpr bool AHI = NP < 3;                            // the weights' hi fragments only (NP 2: the lo ones are zero)
    constexpr int NHL = F16 ? 1 : 2;                        // halves of the B (activation) operand fetched per fragment
    constexpr int NHA = AHI ? 1 : 2;                        // halves of the A (weight) operand fetched per fragment
    constexpr int SLOT = G5_CA * MT * 2 * 1024;            // bytes of a ring slot: [u][m][hl][lane][16 B]
    // three separate arrays, not one: the compiler's wait-count pass then knows that an LDS-DMA into one slot cannot
    // alias the fragment reads of another and puts no vmcnt(0) in front of them
    __shared__ __attribute__((aligned(16))) char ring0[SLOT];
    __shared__ __attribute__((aligned(16))) char ring1[SLOT];
    __shared__ __attribute__((aligned(16))) char ring2[SLOT];
    auto ring = [&](auto slot_) -> char * {
        constexpr int slot = decltype(slot_)::value;
        if constexpr (slot == 0) return ring0;
        else if constexpr (slot == 1) return ring1;
        else return ring2;
    };
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, kg = lane >> 5;
    int id = blockIdx.x;
    const int total = gridDim.x;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    const int split = id % a.splits;
    id /= a.splits;
    const int mb = id % a.MB;
    const int tile = id / a.MB;
    const int tp = tile % a.tiles;
    const int n = tile / a.tiles;
    const int64_t p0 = (int64_t)tp * GM_PIX;
    const int64_t plane = a.P * 16;
    const int ck0 = split * a.sks * GM_KC;                 // first 16-k chunk of this workgroup
    const int nall = a.CK - ck0;
    const int nck = nall < a.sks * GM_KC ? nall : a.sks * GM_KC;
    const int nchunk = (nck + G5_CA - 1) / G5_CA;

    // B: this lane's fragment of column block j, hi / lo, for chunk ck.  The address is split into a WAVE-UNIFORM 64-bit
    // part (sample, chunk, plane, column tile, wave: scalar registers, scalar arithmetic) and ONE loop-invariant 32-bit
    // per-lane offset (kg and the lane's column), i.e. the saddr form of global_load_dwordx4 -- the compiler otherwise keeps
    // a 64-bit VGPR pointer per load of the unrolled trip (48 of them) and the two-product instantiation spilled.
    const char *bbase = a.xs + (((int64_t)n * a.CK + ck0) * 4) * plane + (p0 + (int64_t)wave * 64) * 16;
    const unsigned bvoff = (unsigned)(kg * 2) * (unsigned)plane + (unsigned)l32 * 16u;     // < 2^32: P <= 2^26 columns
    h16x8 Bq[G5_DB][2][NHL];
    auto load_b = [&](int ck, auto slot_) {
        constexpr int slot = decltype(slot_)::value;
        const char *cb = bbase + (int64_t)ck * 4 * plane;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int hl = 0; hl < NHL; ++hl)
                Bq[slot][j][hl] = *reinterpret_cast<const h16x8 *>(cb + (int64_t)hl * plane + j * 512 + bvoff);
    };
    // A: ring slot `slot` <- 16-k chunks c*CA .. c*CA+CA-1 of the MT row blocks; piece q = (u*MT + m)*2 + hl.  The slot
    // is a compile-time constant so that the DMA provably does not alias the fragment reads of the other slots.
    auto issue_a = [&](int c, auto slot_, bool always = false) {
        constexpr int slot = decltype(slot_)::value;
        if (always || c < nchunk) {
#pragma unroll
            for (int q0 = 0; q0 < G5_CA * MT * NHA; q0 += 4) {
                const int qq = q0 + wave;                    // AHI: the hi pieces only, spread over the four waves
                const int q = AHI ? qq * 2 : qq;
                const int hl = q & 1, m = (q >> 1) % MT, u = (q >> 1) / MT;
                int ck = c * G5_CA + u;
                if (ck >= nck) ck = nck - 1;                 // partial last chunk: a valid address, never multiplied
                if (!AHI || qq < G5_CA * MT)
                    glds16b(a.wp + ((((int64_t)(mb * MT + m) * a.CK + ck0 + ck) * 2 + hl) * 1024) + lane * 16,
                            ring(slot_) + q * 1024);
            }
        }
    };

    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

    issue_a(0, cic<0>{});
    issue_a(1, cic<1>{});
    cv_static_for<G5_DB>([&](auto d) { if (d.value < nck) load_b(d.value, d); });
    // ring slots 0 and 1 are in LDS once this wave's loads issued before B(0) have returned and every wave says so
    if (nck >= G5_DB) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NHL * (G5_DB - 1)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");

    // 12 chunks of 16 k = 3 ring slots = 2 rounds of the B registers per trip, everything indexed statically.  The main
    // loop has NO branches (every trip issues all of its loads and DMAs): the compiler's wait-count pass then keeps exact
    // counts (s_waitcnt vmcnt(20): the 20 younger B loads stay in flight); with a branch in the body it merges the
    // pending-load states into vmcnt(0) and drains the queue.  The last trips run the guarded copy of the same steps.
    // SWAP (operand sink of kind 2: attention V fragments; its own launch): the MFMA operands trade places, so the
    // accumulators hold the TRANSPOSED tile -- lane = row of the weight tile, registers = the 32 tokens of column block j
    // -- which is the key order of the attention kernel's V fragments; same three products, same roundings per element.
    auto step = [&](int base, auto t_, auto guarded_) {
        constexpr int t = decltype(t_)::value;
        constexpr bool guarded = decltype(guarded_)::value != 0;
        constexpr int slot = t / G5_CA, u = t % G5_CA, bs = t % G5_DB;
        const int ck = base + t;
        if (guarded && ck >= nck) return;
        if constexpr (u == 0) issue_a(ck / G5_CA + 2, cic<(slot + 2) % 3>{}, !guarded);   // main loop: chunk +2 exists
        const char *ab = ring(cic<slot>{}) + lane * 16;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const h16x8 ah = *reinterpret_cast<const h16x8 *>(ab + ((u * MT + m) * 2 + 0) * 1024);
            h16x8 al;
            if constexpr (NP == 3) al = *reinterpret_cast<const h16x8 *>(ab + ((u * MT + m) * 2 + 1) * 1024);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // products in the order hi.hi, hi.lo (NP >= 2), lo.hi (NP == 3: with NP == 2 the weights' lo half is zero
                // and this product would add exact zeros); SWAP trades the MFMA operands (transposed accumulator)
                if constexpr (SWAP) {
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bq[bs][j][0], ah, acc[m][j], 0, 0, 0);
                    if constexpr (NP >= 2) acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bq[bs][j][NHL - 1], ah, acc[m][j], 0, 0, 0);
                    if constexpr (NP == 3) acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bq[bs][j][0], al, acc[m][j], 0, 0, 0);
                } else {
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, Bq[bs][j][0], acc[m][j], 0, 0, 0);
                    if constexpr (NP >= 2) acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, Bq[bs][j][NHL - 1], acc[m][j], 0, 0, 0);
                    if constexpr (NP == 3) acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, Bq[bs][j][0], acc[m][j], 0, 0, 0);
                }
            }
        }
        // the scheduler otherwise gathers the loads of several steps into one cluster late in the chunk, which shortens
        // the prefetch distance and turns the counted waits into vmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
        if (!guarded || ck + G5_DB < nck) load_b(ck + G5_DB, cic<bs>{});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (u == G5_CA - 1) asm volatile("s_barrier" ::: "memory");   // slot free for chunk +3, chunk +1 landed
    };
    int base = 0;
    for (; base + 12 + G5_DB <= nck; base += 12) cv_static_for<12>([&](auto t_) { step(base, t_, cic<0>{}); });
    for (; base < nck; base += 12) cv_static_for<12>([&](auto t_) { step(base, t_, cic<1>{}); });
    if constexpr (SWAP) gemm_epilogue_vfrag<MT>(a, acc, n, mb, p0, wave, lane);
    else
    gemm_epilogue<MT, true>(a, acc, n, mb, p0, split, wave, lane);
}

// ---- the same GEMM with a square-ish workgroup tile ---------------------------------------------------------
// At split-precision MFMA rates the kernel above is bound by L2 -> LDS operand traffic, not by the matrix pipe: a
// workgroup tile of Tm x Tp needs (Tm + Tp) / (Tm Tp) x 2731 B/clk/CU of operands to keep the pipe busy, i.e. 96
// B/clk for 32 x 256 and 53 B/clk for 64 x 256 against ~55 B/clk/CU of L2 bandwidth.  Here a workgroup owns
// (WGM*64) x (WGP*64) outputs (128 x 256: 32 B/clk), every wave a 64 x 64 block (2 x 2 MFMA tiles, 12 MFMAs per
// eight fragment reads), operands of one 32-deep k-stage land by DMA NST-1 stages ahead of their use and the wave
// waits with a COUNTED vmcnt for exactly the stage it is about to read.
template <int WGM, int WGP, int NST>
__global__ void __launch_bounds__(WGM * WGP * 64) gemm2_f16x3_kernel(const GemmArgs a) {
    constexpr int NW = WGM * WGP;
    constexpr int TP = WGP * 64;
    constexpr int AB = WGM * 2 * GM_KC * 2 * 1024;          // A stage: [m-tile][kc][hl][lane][16 B]
    constexpr int BB = GM_KC * 4 * TP * 16;                 // B stage: [kc][kg*2+hl][column][16 B]
    constexpr int NAP = AB / 1024, NBP = BB / 1024;
    constexpr int PPW = (NAP + NBP) / NW;                   // DMA pieces per wave per stage
    static_assert((NAP + NBP) % NW == 0, "pieces must divide evenly over the waves (counted vmcnt)");
    constexpr int AHEAD = NST - 1;
    constexpr int WAITN = PPW * (AHEAD - 1);                // pieces that may still be in flight when a stage is read
    static_assert(WAITN < 64, "vmcnt field");
    __shared__ __attribute__((aligned(16))) char lds[NST * (AB + BB)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, kg = lane >> 5;
    const int wm = wave % WGM, wp = wave / WGM;
    int id = blockIdx.x;
    const int total = gridDim.x;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    const int mb = id % a.MB;
    const int tile = id / a.MB;
    const int tp = tile % a.tiles;
    const int n = tile / a.tiles;
    const int64_t p0 = (int64_t)tp * TP;
    const int64_t plane = a.P * 16;
    const char *xs_n = a.xs + (int64_t)n * a.CK * 4 * plane + (p0 + lane) * 16;
    const char *wp_b = a.wp + (int64_t)mb * (WGM * 2) * a.CK * 2048 + lane * 16;

    auto issue = [&](int s, int buf) {
        char *ad = lds + buf * (AB + BB), *bd = ad + AB;
#pragma unroll
        for (int q0 = 0; q0 < NAP + NBP; q0 += NW) {
            const int q = q0 + wave;
            if (q < NAP) {                                  // q = (mt * GM_KC + kc) * 2 + hl
                const int hl = q & 1, kc = (q >> 1) % GM_KC, mt = (q >> 1) / GM_KC;
                glds16b(wp_b + (((int64_t)mt * a.CK + s * GM_KC + kc) * 2 + hl) * 1024, ad + q * 1024);
            } else {                                        // r = (kc * 4 + piece) * WGP + column block
                const int r = q - NAP;
                const int cb = r % WGP, pl = r / WGP;       // pl = kc * 4 + (kg * 2 + hl)
                glds16b(xs_n + ((int64_t)(s * GM_KC * 4 + pl)) * plane + cb * 1024, bd + (pl * TP + cb * 64) * 16);
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

    const int nstage = a.CK / GM_KC;
#pragma unroll
    for (int s = 0; s < AHEAD; ++s)
        if (s < nstage) issue(s, s);
    for (int s = 0; s < nstage; ++s) {
        // stage s has landed once at most the pieces of the AHEAD-1 younger stages are outstanding
        if (s + AHEAD - 1 < nstage) __builtin_amdgcn_s_waitcnt(0x0f70 | (WAITN & 15) | ((WAITN >> 4) << 14));
        else __builtin_amdgcn_s_waitcnt(0x0f70);
        __syncthreads();                                   // everyone's pieces; everyone is done with stage s-1
        if (s + AHEAD < nstage) issue(s + AHEAD, (s + AHEAD) % NST);
        const char *ab = lds + (s % NST) * (AB + BB) + lane * 16, *bb = lds + (s % NST) * (AB + BB) + AB;
#pragma unroll
        for (int kc = 0; kc < GM_KC; ++kc) {
            h16x8 bh[2], bl[2], ah[2], al[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = (wp * 2 + j) * 32 + l32;
                bh[j] = *reinterpret_cast<const h16x8 *>(bb + ((kc * 4 + kg * 2 + 0) * TP + col) * 16);
                bl[j] = *reinterpret_cast<const h16x8 *>(bb + ((kc * 4 + kg * 2 + 1) * TP + col) * 16);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                ah[m] = *reinterpret_cast<const h16x8 *>(ab + (((wm * 2 + m) * GM_KC + kc) * 2 + 0) * 1024);
                al[m] = *reinterpret_cast<const h16x8 *>(ab + (((wm * 2 + m) * GM_KC + kc) * 2 + 1) * 1024);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bh[j], acc[m][j], 0, 0, 0);
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bl[j], acc[m][j], 0, 0, 0);
                    acc[m][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[m], bh[j], acc[m][j], 0, 0, 0);
                }
        }
    }
    const float inv = a.w_scale2[1] * (a.x_scale2 ? a.x_scale2[1] : 1.f);
    // loads of the epilogue issued together, ahead of the arithmetic (see the convolution's epilogue)
    const bool hb = a.bias != nullptr, hc = a.chan_add != nullptr, hr = a.residual != nullptr;
    auto out_index = [&](int m, int j, int r, int &row) -> int64_t {
        row = ((mb * WGM + wm) * 2 + m) * 32 + 8 * (r >> 2) + 4 * kg + (r & 3);
        return ((int64_t)n * a.M + row) * a.P + p0 + (wp * 2 + j) * 32 + l32;
    };
    float bv[2][16], cv[2][16];
    f32x16 rv[2][2];
    if (hr) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { int row; rv[m][j][r] = a.residual[out_index(m, j, r, row)]; }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ((mb * WGM + wm) * 2 + m) * 32 + 8 * (r >> 2) + 4 * kg + (r & 3);
            bv[m][r] = hb ? a.bias[row] : 0.f;
            cv[m][r] = hc ? a.chan_add[(int64_t)n * a.M + row] : 0.f;
        }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row;
                const int64_t o = out_index(m, j, r, row);
                float v = acc[m][j][r] * inv;
                if (hb) v += bv[m][r];
                if (hc) v += cv[m][r];
                if (hr) v += rv[m][j][r];
                a.y[o] = v;
            }
}

}  // namespace mvip

using namespace mvip;

extern "C" int64_t mvip_gemm_packed_bytes(int64_t M, int64_t K) {
    if (M <= 0 || K <= 0) return 0;
    return M * K * 4 + 256;
}

extern "C" int mvip_gemm_pack_a(const float *src, int64_t M, int64_t K, int64_t sm, int64_t sk, void *packed,
                                void *stream) {
    if (!src || !packed || M <= 0 || M % 32 != 0 || K <= 0 || K % 32 != 0) return MVIP_EINVAL;
    hipStream_t st = as_stream(stream);
    char *tail = (char *)packed + M * K * 4;
    zero_words(tail, 64, st);
    // maximum + scale in one launch: its two scratch words (tail + 16, + 20) are zero on entry and left zero
    launch_absmax_scale(src, M * K, (unsigned *)(tail + 16), (float *)tail, st);
    const int64_t total = (M / 32) * (K / 16) * 2 * 64;
    hipLaunchKernelGGL(gm_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, (int)M, (int)K, sm,
                       sk, (const float *)tail, (uint4 *)packed, (unsigned *)(tail + 12));
    return check_launch();
}

// splits for the 32/64-row kernel: only grids under 3/4 of the chip, at least 16 stages (512 k) per workgroup -- with
// shorter contractions the second launch costs more than the idle CUs did (measured, tools/gemm_bench.py: K = 640 at
// 160 workgroups 15.7 -> 21.2 us with splits, K = 5120 at 80 workgroups 97.6 -> 46.4 us)
static inline int gm_splits(int64_t blocks, int64_t nstage) {
    static const int forced = [] { const char *e = getenv("MVIP_GEMM_SPLITS"); return e ? atoi(e) : 0; }();   // tuning
    int64_t s = forced > 0 ? forced : (blocks >= 192 ? 1 : (384 + blocks - 1) / blocks);
    if (s > nstage / 16) s = nstage / 16;
    if (s > 32) s = 32;
    if (s < 1) s = 1;
    const int64_t sks = (nstage + s - 1) / s;
    return (int)((nstage + sks - 1) / sks);
}
// row tiles per workgroup of the 32/64-row kernels: cv_mt's choice, or (MVIP_GEMM_MT2=1, experiment) 64 rows whenever M allows
static inline int gm_mt(int64_t M, int64_t tiles) {
    static const int mt2_env = [] { const char *e = getenv("MVIP_GEMM_MT2"); return e ? atoi(e) : 0; }();
    const int mt = cv_mt(M, tiles);
    return (mt2_env && mt == 1 && M % 64 == 0) ? 2 : mt;
}
static inline int gm_auto_cfg(int64_t N, int64_t M, int64_t P) {
    // Measured on the UNet's linear layers (tools/gemm_bench.py, profiles/r2_gemm_tiles.json): with K = 320..1280
    // (10..40 stages) every tile shape lands within ~10 % of the 32/64-row kernel -- these launches are bound by
    // the per-workgroup prologue / epilogue and by grid quantisation, not by operand traffic -- and the square
    // tile only wins once M is large enough for several full waves of workgroups (the 1280-wide GEGLU projection).
    return (M % 128 == 0 && M >= 8192 && (M / 128) * N * (P / 256) >= 128) ? 2 : 1;
}

extern "C" int64_t mvip_gemm_workspace_bytes(int64_t N, int64_t K, int64_t M, int64_t P) {
    if (N <= 0 || M <= 0 || M % 32 != 0 || K <= 0 || K % 32 != 0 || P <= 0 || P % GM_PIX != 0 || P > GM_P_MAX) return 0;
    if (gm_auto_cfg(N, M, P) != 1) return 0;
    const int64_t tiles = P / GM_PIX;
    const int MT = gm_mt(M, N * tiles);
    const int s = gm_splits(N * tiles * (M / (32 * MT)), K / 32);
    return s > 1 ? (int64_t)s * N * M * P * 4 : 0;
}

static int gemm_launch(const void *xs, const void *packed, const float *bias, const float *chan_add,
                       const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                       float *y, int cfg, void *workspace, int prec, void *stream, double *ln_part = nullptr) {
    if (N < 0 || M <= 0 || M % 32 != 0 || K <= 0 || K % 32 != 0 || P <= 0 || P % GM_PIX != 0 || P > GM_P_MAX || prec < 0 || prec > 2)
        return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!xs || !packed || !y) return MVIP_EINVAL;
    GemmArgs a;
    a.xs = (const char *)xs; a.wp = (const char *)packed;
    a.w_scale2 = (const float *)((const char *)packed + M * K * 4);
    a.bias = bias; a.chan_add = chan_add; a.residual = residual; a.x_scale2 = x_scale2; a.y = y;
    a.N = (int)N; a.CK = (int)(K / 16); a.M = (int)M; a.P = P;
    a.geglu_L = 0; a.absmax_bits = nullptr; a.nsec = 0; a.v_dt = 1; a.prec = prec;
    a.splits = 1; a.ln_part = nullptr; a.sks = (int)(K / 32); a.partial = nullptr;
#ifdef MVIP_EXPERIMENT_GEMM
    a.dbg = cfg >> 8; cfg &= 255;
#endif
    hipStream_t st = as_stream(stream);
    const bool auto_cfg = cfg == 0;
    if (cfg == 0) cfg = prec ? 1 : gm_auto_cfg(N, M, P);     // the one- / two-product instantiations exist for the 32/64-row kernel
    // prec 1 (fp16 mode): the producers wrote NO lo planes, so a three-product kernel would read uninitialised halves --
    // refuse every configuration without a single-product instantiation (prec 2 may fall back: the result is identical)
    if (prec == 1 && (cfg == 2 || cfg == 3 || cfg == 4)) return MVIP_EUNSUP;
    if (cfg < 0 || cfg > 5) return MVIP_EINVAL;
    if ((cfg == 2 || cfg == 3) && M % 128 != 0) return MVIP_EINVAL;
    if (cfg == 4 && M % 64 != 0) return MVIP_EINVAL;
    if (ln_part && cfg != 1 && cfg != 5) return MVIP_EUNSUP;   // the 32/64-row kernels' epilogue only
    if (cfg == 2) {
        a.tiles = (int)(P / 256); a.MB = (int)(M / 128);
        hipLaunchKernelGGL((gemm2_f16x3_kernel<2, 4, 3>), dim3((unsigned)(N * a.tiles * a.MB)), dim3(512), 0, st, a);
    } else if (cfg == 3) {
        a.tiles = (int)(P / 128); a.MB = (int)(M / 128);
        hipLaunchKernelGGL((gemm2_f16x3_kernel<2, 2, 2>), dim3((unsigned)(N * a.tiles * a.MB)), dim3(256), 0, st, a);
    } else if (cfg == 4) {
        a.tiles = (int)(P / 128); a.MB = (int)(M / 64);
        hipLaunchKernelGGL((gemm2_f16x3_kernel<1, 2, 3>), dim3((unsigned)(N * a.tiles * a.MB)), dim3(128), 0, st, a);
    } else {
        a.tiles = (int)(P / GM_PIX);
        const int MT = gm_mt(M, N * a.tiles);
        a.MB = (int)(M / (32 * MT));
        int64_t blocks = N * a.tiles * a.MB;
        if (workspace && auto_cfg) {
            a.splits = gm_splits(blocks, K / 32);
            if (a.splits > 1) { a.sks = (int)((K / 32 + a.splits - 1) / a.splits); a.partial = (float *)workspace; }
        }
        blocks *= a.splits;
        if (blocks > 0x7fffffffLL) return MVIP_EINVAL;
        // cfg 5 (and the automatic choice unless MVIP_GEMM_STREAM=0): the B-in-registers kernel
        static const bool stream_env = [] { const char *e = getenv("MVIP_GEMM_STREAM"); return e ? atoi(e) != 0 : true; }();
        const bool stream = cfg == 5 || (auto_cfg && stream_env);
        if (ln_part && (a.splits > 1 || !stream || MT > 2)) return MVIP_EUNSUP;       // callers ask mvip_gemm_ln_segments first
        a.ln_part = ln_part;
        if (prec == 1 && !(MT <= 2 && stream)) return MVIP_EUNSUP;             // (see above: no lo planes in fp16 mode)
        if (prec == 1) {
            if (MT == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((gemm5_f16x3_kernel<1, false, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        } else if (prec == 2 && MT <= 2 && stream) {
            if (MT == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
            else hipLaunchKernelGGL((gemm5_f16x3_kernel<1, false, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        } else if (MT == 4)
            hipLaunchKernelGGL((gemm_f16x3_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else if (MT == 2 && stream)
            hipLaunchKernelGGL((gemm5_f16x3_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else if (MT == 2)
            hipLaunchKernelGGL((gemm_f16x3_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else if (stream)
            hipLaunchKernelGGL((gemm5_f16x3_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((gemm_f16x3_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        if (a.partial) launch_split_reduce(a.partial, a.splits, N * M, (int)M, P, a.w_scale2, x_scale2, bias, chan_add, residual, y, st);
    }
    return check_launch();
}

// cfg: 0 = choose by shape, 1 = 32/64-row kernel (operands through LDS), 2 = 128 x 256 tile, 3 = 128 x 128, 4 = 64 x 128,
// 5 = 32/64-row kernel with the B operand streamed into registers (timing switch)
extern "C" int mvip_gemm_f16x3_cfg(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                   const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                                   float *y, int cfg, int prec, void *stream) {
    return gemm_launch(xs, packed, bias, chan_add, residual, x_scale2, N, K, M, P, y, cfg, nullptr, prec, stream);
}

extern "C" int mvip_gemm_f16x3(const void *xs, const void *packed, const float *bias, const float *chan_add,
                               const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                               float *y, int prec, void *stream) {
    return gemm_launch(xs, packed, bias, chan_add, residual, x_scale2, N, K, M, P, y, 0, nullptr, prec, stream);
}

// mvip_gemm_f16x3 with a caller-owned workspace of mvip_gemm_workspace_bytes(N, K, M, P) bytes (null when that is 0):
// launches with fewer than one workgroup per CU and a long contraction (the 1280-channel transformer blocks at 16 x 16:
// 80 workgroups x 160 stages) are split over K and summed by a second launch, in index order.
extern "C" int mvip_gemm_f16x3_ws(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                  const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                                  float *y, void *workspace, int prec, void *stream) {
    if (!workspace && mvip_gemm_workspace_bytes(N, K, M, P) > 0) return MVIP_EINVAL;
    return gemm_launch(xs, packed, bias, chan_add, residual, x_scale2, N, K, M, P, y, 0, workspace, prec, stream);
}

// Segments (= workgroup row blocks of 32 or 64 rows) of the LayerNorm partial statistics mvip_gemm_f16x3_ws_ln leaves for
// this shape, or 0 when the launch cannot leave them (split-K launches sum raw partial products in a second launch; the
// square-tile kernel has an epilogue of its own): the caller then runs mvip_layernorm_split_planes' own statistics pass.
extern "C" int64_t mvip_gemm_ln_segments(int64_t N, int64_t K, int64_t M, int64_t P, int prec) {
    if (N <= 0 || M <= 0 || M % 32 != 0 || K <= 0 || K % 32 != 0 || P <= 0 || P % GM_PIX != 0 || P > GM_P_MAX || prec < 0 || prec > 2) return 0;
    if ((prec ? 1 : gm_auto_cfg(N, M, P)) != 1) return 0;
    const int64_t tiles = P / GM_PIX;
    const int MT = gm_mt(M, N * tiles);
    if (gm_splits(N * tiles * (M / (32 * MT)), K / 32) > 1) return 0;
    static const bool stream_env = [] { const char *e = getenv("MVIP_GEMM_STREAM"); return e ? atoi(e) != 0 : true; }();
    if (MT > 2 || !stream_env) return 0;               // the statistics live in the B-in-registers kernel's epilogue
    return M / (32 * MT);
}

// mvip_gemm_f16x3_ws that ALSO leaves the LayerNorm statistics of its output over the M rows (DS_NeRF/guidance/sd_utils.py:390-403:
// the unet(...) call -- BasicTransformerBlock's norm1 / norm2 / norm3 read the residual stream a projection just wrote): per
// column p and segment g (mvip_gemm_ln_segments of them) the fp64 sum and sum of squares of the finished rows of the
// segment, ln_part[((n * S + g) * 2 + {0, 1}) * P + p] -- what mvip_layernorm_split_planes_stats consumes.  N * S * 2 * P doubles.
extern "C" int mvip_gemm_f16x3_ws_ln(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                     const float *residual, const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P,
                                     float *y, void *workspace, void *ln_part, int prec, void *stream) {
    if (!ln_part || mvip_gemm_ln_segments(N, K, M, P, prec) == 0) return MVIP_EINVAL;
    return gemm_launch(xs, packed, bias, chan_add, residual, x_scale2, N, K, M, P, y, 0, workspace, prec, stream, (double *)ln_part);
}

// First projection of the transformer feed-forward with the GEGLU fused into the epilogue:
//   out[n][r][p] = (W_v x + b_v)[r] * gelu((W_g x + b_g)[r])   for p < L, zero beyond,
// `packed` / `bias` hold the 2R rows interleaved in 32-row tiles (value rows 32 t .. 32 t + 31, then the gate rows of
// the same t); scale2 receives the power-of-two scale of |out|max; zero_word as in mvip_absmax_scale_sections.
extern "C" int mvip_gemm_geglu_f16x3(const void *xs, const void *packed, const float *bias, const float *x_scale2,
                                     int64_t N, int64_t K, int64_t M2, int64_t P, int64_t L, float *out, float *scale2,
                                     void *zero_word, int prec, void *stream) {
    if (prec < 0 || prec > 2 || N < 0 || M2 <= 0 || M2 % 64 != 0 || K <= 0 || K % 32 != 0 || P <= 0 || P % GM_PIX != 0 || P > GM_P_MAX || L <= 0 || L > P ||
        !scale2 || !zero_word)
        return MVIP_EINVAL;
    hipStream_t st = as_stream(stream);
    if (N > 0) {
        if (!xs || !packed || !out) return MVIP_EINVAL;
        GemmArgs a;
        a.xs = (const char *)xs; a.wp = (const char *)packed;
        a.w_scale2 = (const float *)((const char *)packed + M2 * K * 4);
        a.bias = bias; a.chan_add = nullptr; a.residual = nullptr; a.x_scale2 = x_scale2; a.y = out;
        a.N = (int)N; a.CK = (int)(K / 16); a.M = (int)M2; a.P = P; a.tiles = (int)(P / GM_PIX); a.MB = (int)(M2 / 64);
        a.geglu_L = (int)L; a.absmax_bits = (unsigned *)zero_word; a.nsec = 0; a.v_dt = 1; a.prec = prec;
        a.splits = 1; a.ln_part = nullptr; a.sks = (int)(K / 32); a.partial = nullptr;
        const int64_t blocks = N * a.tiles * a.MB;
        if (blocks > 0x7fffffffLL) return MVIP_EINVAL;
        static const bool stream_env = [] { const char *e = getenv("MVIP_GEMM_STREAM"); return e ? atoi(e) != 0 : true; }();
        if (prec == 1) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else if (prec == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else if (stream_env) hipLaunchKernelGGL((gemm5_f16x3_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gemm_f16x3_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(scale_from_bits_kernel, dim3(1), dim3(1), 0, st, scale2, (unsigned *)zero_word);
    return check_launch();
}

// ---- GEMMs whose epilogue writes the NEXT contraction's operands (csrc/plane_sink.h) ------------------------------
// The M rows are cut into `nsec` <= 3 consecutive sections of sec_rows[i] rows (multiples of 64).  Section i goes to
// sec_ptr[i] in the format sec_kind[i] -- 1: split planes [N][sec_rows/16][2][2][P][8 halves] (the B operand of a later
// mvip_gemm_f16x3 / the Q or K operand of the attention kernel), 2: attention V fragments
// [N][heads][v_dt][P/16][2][64][8 halves] with sec_rows = heads * v_dt * 32 (rows of head h at h * v_dt * 32 ..) -- as
// (W x + bias) * sec_scale[i], sec_scale a power of two the caller fixed BEFORE the launch from a bound of the result.
extern "C" int mvip_gemm_f16x3_sinks(const void *xs, const void *packed, const float *bias, const float *x_scale2, int64_t N,
                                     int64_t K, int64_t M, int64_t P, int nsec, const int64_t *sec_rows, const int *sec_kind,
                                     void *const *sec_ptr, const float *sec_scale, int v_dt, int prec, void *stream) {
    if (prec < 0 || prec > 2 || N < 0 || M <= 0 || M % 64 != 0 || K <= 0 || K % 32 != 0 || P <= 0 || P % GM_PIX != 0 || P > GM_P_MAX || nsec < 1 || nsec > 3 ||
        !sec_rows || !sec_kind || !sec_ptr || !sec_scale)
        return MVIP_EINVAL;
    int64_t end = 0, plane_rows = 0;
    int n_plane = 0;
    for (int i = 0; i < nsec; ++i) {
        if (sec_rows[i] <= 0 || sec_rows[i] % 64 != 0 || (sec_kind[i] != 1 && sec_kind[i] != 2) || !(sec_scale[i] > 0.f))
            return MVIP_EINVAL;
        // the plane sections come first; a V-fragment section (computed by the transposed instantiation, its own launch)
        // is the last one
        if (sec_kind[i] == 2 && (i != nsec - 1 || v_dt < 1 || sec_rows[i] % (32 * (int64_t)v_dt) != 0)) return MVIP_EINVAL;
        if (sec_kind[i] == 1) { plane_rows += sec_rows[i]; ++n_plane; }
        end += sec_rows[i];
    }
    if (end != M) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!xs || !packed) return MVIP_EINVAL;
    for (int i = 0; i < nsec; ++i) if (!sec_ptr[i]) return MVIP_EINVAL;
    hipStream_t st = as_stream(stream);
    GemmArgs a;
    a.xs = (const char *)xs;
    a.w_scale2 = (const float *)((const char *)packed + M * K * 4);
    a.chan_add = nullptr; a.residual = nullptr; a.x_scale2 = x_scale2; a.y = nullptr;
    a.N = (int)N; a.CK = (int)(K / 16); a.P = P;
    a.geglu_L = 0; a.absmax_bits = nullptr; a.v_dt = v_dt < 1 ? 1 : v_dt; a.prec = prec;
    a.splits = 1; a.ln_part = nullptr; a.sks = (int)(K / 32); a.partial = nullptr;
#ifdef MVIP_EXPERIMENT_GEMM
    a.dbg = 0;
#endif
    a.tiles = (int)(P / GM_PIX);
    auto launch = [&](int64_t row0, int64_t rows, bool swap) -> int {
        a.wp = (const char *)packed + row0 * K * 4;          // row tiles are contiguous in the packed image
        a.bias = bias ? bias + row0 : nullptr;
        a.M = (int)rows;
        const int MT = cv_mt(rows, N * a.tiles) >= 2 ? 2 : 1;
        a.MB = (int)(rows / (32 * MT));
        const int64_t blocks = N * a.tiles * a.MB;
        if (blocks > 0x7fffffffLL) return MVIP_EINVAL;
#define MVIP_G5(MT_, SW_)                                                                                                    \
        do {                                                                                                                    \
            if (prec == 1) hipLaunchKernelGGL((gemm5_f16x3_kernel<MT_, SW_, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a);  \
            else if (prec == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<MT_, SW_, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a); \
            else hipLaunchKernelGGL((gemm5_f16x3_kernel<MT_, SW_, 3>), dim3((unsigned)blocks), dim3(256), 0, st, a);            \
        } while (0)
        if (swap) { if (MT == 2) MVIP_G5(2, true); else MVIP_G5(1, true); }
        else { if (MT == 2) MVIP_G5(2, false); else MVIP_G5(1, false); }
#undef MVIP_G5
        return MVIP_OK;
    };
    for (int i = 0; i < 3; ++i) { a.sec[i].ptr = nullptr; a.sec[i].scale = 1.f; a.sec[i].row_end = 0; a.sec[i].kind = 0; }
    if (n_plane > 0) {
        int64_t e = 0;
        for (int i = 0; i < n_plane; ++i) {
            e += sec_rows[i];
            a.sec[i].ptr = (char *)sec_ptr[i]; a.sec[i].scale = sec_scale[i]; a.sec[i].row_end = (int)e; a.sec[i].kind = 1;
        }
        a.nsec = n_plane;
        const int rc = launch(0, plane_rows, false);
        if (rc != MVIP_OK) return rc;
    }
    if (n_plane < nsec) {
        for (int i = 0; i < 3; ++i) { a.sec[i].ptr = nullptr; a.sec[i].scale = 1.f; a.sec[i].row_end = 0; a.sec[i].kind = 0; }
        a.sec[0].ptr = (char *)sec_ptr[nsec - 1]; a.sec[0].scale = sec_scale[nsec - 1]; a.sec[0].row_end = (int)sec_rows[nsec - 1];
        a.sec[0].kind = 2;
        a.nsec = 1;
        const int rc = launch(plane_rows, sec_rows[nsec - 1], true);
        if (rc != MVIP_OK) return rc;
    }
    return check_launch();
}

// mvip_gemm_geglu_f16x3 whose product leaves as the second projection's operand planes [N][(M2/2)/16][2][2][P][8 halves],
// times the power of two `out_scale` fixed before the launch (|value * gelu(gate)| <= |value| |gate|): no absolute-maximum
// collection, no scale launch, no fp32 intermediate.
extern "C" int mvip_gemm_geglu_f16x3_sink(const void *xs, const void *packed, const float *bias, const float *x_scale2,
                                          int64_t N, int64_t K, int64_t M2, int64_t P, int64_t L, void *out_planes,
                                          float out_scale, int prec, void *stream) {
    if (prec < 0 || prec > 2 || N < 0 || M2 <= 0 || M2 % 64 != 0 || K <= 0 || K % 32 != 0 || P <= 0 || P % GM_PIX != 0 || P > GM_P_MAX || L <= 0 || L > P ||
        !(out_scale > 0.f) || (M2 / 2) % 16 != 0)
        return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!xs || !packed || !out_planes) return MVIP_EINVAL;
    GemmArgs a;
    a.xs = (const char *)xs; a.wp = (const char *)packed;
    a.w_scale2 = (const float *)((const char *)packed + M2 * K * 4);
    a.bias = bias; a.chan_add = nullptr; a.residual = nullptr; a.x_scale2 = x_scale2; a.y = nullptr;
    a.N = (int)N; a.CK = (int)(K / 16); a.M = (int)M2; a.P = P; a.tiles = (int)(P / GM_PIX); a.MB = (int)(M2 / 64);
    a.geglu_L = (int)L; a.absmax_bits = nullptr; a.nsec = 1; a.v_dt = 1; a.prec = prec;
    for (int i = 0; i < 3; ++i) { a.sec[i].ptr = nullptr; a.sec[i].scale = 1.f; a.sec[i].row_end = 0; a.sec[i].kind = 0; }
    a.sec[0].ptr = (char *)out_planes; a.sec[0].scale = out_scale; a.sec[0].row_end = (int)(M2 / 2); a.sec[0].kind = 1;
    a.splits = 1; a.ln_part = nullptr; a.sks = (int)(K / 32); a.partial = nullptr;
#ifdef MVIP_EXPERIMENT_GEMM
    a.dbg = 0;
#endif
    const int64_t blocks = N * a.tiles * a.MB;
    if (blocks > 0x7fffffffLL) return MVIP_EINVAL;
    if (prec == 1) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 1>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
    else if (prec == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 2>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL((gemm5_f16x3_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
    return check_launch();
}

// Y = (W X + bias + residual) * out_scale as ONE section of split planes [N][M/16][2][2][P][8 halves] -- the operand of
// the next GEMM (the second feed-forward projection handing the residual stream to proj_out) -- with the split-K of
// mvip_gemm_f16x3_ws: workspace of mvip_gemm_workspace_bytes(N, K, M, P) bytes (null when that is 0).
extern "C" int mvip_gemm_f16x3_planes_ws(const void *xs, const void *packed, const float *bias, const float *residual,
                                         const float *x_scale2, int64_t N, int64_t K, int64_t M, int64_t P, void *out_planes,
                                         float out_scale, void *workspace, int prec, void *stream) {
    if (prec < 0 || prec > 2 || N < 0 || M <= 0 || M % 32 != 0 || K <= 0 || K % 32 != 0 || P <= 0 || P % GM_PIX != 0 || P > GM_P_MAX || !(out_scale > 0.f))
        return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!xs || !packed || !out_planes) return MVIP_EINVAL;
    if (!workspace && mvip_gemm_workspace_bytes(N, K, M, P) > 0) return MVIP_EINVAL;
    GemmArgs a;
    a.xs = (const char *)xs; a.wp = (const char *)packed;
    a.w_scale2 = (const float *)((const char *)packed + M * K * 4);
    a.bias = bias; a.chan_add = nullptr; a.residual = residual; a.x_scale2 = x_scale2; a.y = nullptr;
    a.N = (int)N; a.CK = (int)(K / 16); a.M = (int)M; a.P = P;
    a.geglu_L = 0; a.absmax_bits = nullptr; a.nsec = 1; a.v_dt = 1; a.prec = prec;
    for (int i = 0; i < 3; ++i) { a.sec[i].ptr = nullptr; a.sec[i].scale = 1.f; a.sec[i].row_end = 0; a.sec[i].kind = 0; }
    a.sec[0].ptr = (char *)out_planes; a.sec[0].scale = out_scale; a.sec[0].row_end = (int)M; a.sec[0].kind = 1;
    a.splits = 1; a.ln_part = nullptr; a.sks = (int)(K / 32); a.partial = nullptr;
#ifdef MVIP_EXPERIMENT_GEMM
    a.dbg = 0;
#endif
    a.tiles = (int)(P / GM_PIX);
    int MT = gm_mt(M, N * a.tiles);
    if (MT > 2) MT = 2;
    a.MB = (int)(M / (32 * MT));
    int64_t blocks = N * a.tiles * a.MB;
    if (workspace && gm_auto_cfg(N, M, P) == 1 && MT == gm_mt(M, N * a.tiles)) {
        a.splits = gm_splits(blocks, K / 32);
        if (a.splits > 1) { a.sks = (int)((K / 32 + a.splits - 1) / a.splits); a.partial = (float *)workspace; }
    }
    blocks *= a.splits;
    if (blocks > 0x7fffffffLL || N * (M / 8) > 65535) return MVIP_EINVAL;
    hipStream_t st = as_stream(stream);
    if (prec == 1) {
        if (MT == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gemm5_f16x3_kernel<1, false, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    } else if (prec == 2) {
        if (MT == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gemm5_f16x3_kernel<1, false, 2>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    } else {
        if (MT == 2) hipLaunchKernelGGL((gemm5_f16x3_kernel<2, false>), dim3((unsigned)blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((gemm5_f16x3_kernel<1, false>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    }
    if (a.partial)
        hipLaunchKernelGGL(cv_split_reduce_planes_kernel, dim3((unsigned)((P + 255) / 256), (unsigned)(N * (M / 8))), dim3(256), 0,
                           st, a.partial, a.splits, (int)N, (int)M, P, a.w_scale2, x_scale2, bias, residual, out_scale,
                           (uint4 *)out_planes, prec);
    return check_launch();
}
