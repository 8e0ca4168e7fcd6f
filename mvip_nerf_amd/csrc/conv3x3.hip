// 3x3 / stride 1 / pad 1 convolution of the SDS networks as an implicit GEMM on the fp16 matrix cores in
// split precision ("f16x3": both operands split into fp16 hi + lo, the three leading products
// Wh.Xh + Wh.Xl + Wl.Xh accumulated in fp32 -- ~1e-6 relative, i.e. fp32-grade results at ~2.7x the
// exact-fp32 MFMA rate).  These are the ResNet-block convolutions inside vae.encode / unet
// (call sites DS_NeRF/guidance/sd_utils.py:148, :162, :189, :212; block structure from the published
// SD-1.5 architecture) -- 1.0 TFLOP per VAE encode, the largest single item of the SDS step.
//
// GEMM view: M = output channels, N = pixels, K = (tap, input channel).
//   * activations arrive in "split planes": xs[n][Cin/16][kg 2][hl 2][H][W][8 halves] -- for 16-channel
//     chunk ck, plane (kg, hl) holds channels ck*16 + kg*8 + 0..7 of every pixel as the hi (hl=0) or lo
//     (hl=1) fp16 term.  16 B per (pixel, plane) = one MFMA B-operand fragment, so a haloed pixel tile goes
//     HBM -> LDS by DMA (global_load_lds) with no register staging, and the shifted windows of the nine
//     taps are plain offset reads of the same LDS tile.  The producers write this layout directly
//     (GroupNorm+SiLU apply, or the plain converter for gradients).
//   * weights are packed once per layer in MFMA A-fragment order, pre-scaled by a power of two so that
//     the lo terms stay in fp16's normal range:
//     wp[Cout/32][Cin/16][ky][kx][hl][lane 64][8 halves]; the tail holds {scale, 1/scale}.
//   * one workgroup = MT*32 output channels x (8 x 32) pixels, 4 waves, each wave MT x 2 accumulator tiles;
//     MT = 4, 2 or 1 is chosen per launch so that the grid covers the 256 CUs.
//     K loop: 16 input channels x one kernel row per stage (3 taps, 72 MFMAs per wave at MT=4), weights
//     and the input tile double-buffered in LDS, one barrier per stage.
//   * epilogue: x 1/scale, + bias, + per-(sample, channel) addend (time embedding), + residual, NCHW fp32.
//   * NP (template; `prec` of the C ABI): products per contraction step.  3 = Wh.Xh + Wh.Xl + Wl.Xh (prec 0); 1 = Wh.Xh only
//     (prec 1, the reference's --fp16 mode); 2 = Wh.Xh + Wh.Xl (prec 2) for weights that are EXACTLY fp16 values -- every
//     weight the reference ever loads is one (DS_NeRF/guidance/sd_utils.py:69-74: `revision="fp16"`, cast up in the default
//     fp32 mode), so the packed image's lo fragments are all zero, the third product adds exact zeros, and leaving it out
//     changes no bit of the result while a third of the matrix work and half of the weight-operand bytes go away.  The
//     packers record whether any lo fragment is non-zero (tail word 12; mvip_packed_weights_two_product reads it).
#include "f16x3_operand.h"
#include <stdlib.h>

namespace mvip {

constexpr int CV_TH = 8, CV_TW = 32;
constexpr int CV_HW = CV_TW + 2;                    // haloed tile width
constexpr int CV_PIX = (CV_TH + 2) * CV_HW;         // 340 haloed pixels of the 8 x 32 tile (4 planes x 340 slots = 21,760 B)

// ---- weight packing ----------------------------------------------------------------------------------
// one thread per 16-byte fragment piece.  transpose = 1 packs the data-gradient operator:
// W'[co'][ci'][ky][kx] = W[ci'][co'][2-ky][2-kx]  (Cout' = Cin, Cin' = Cout of the forward layer).
__global__ void cv_pack_kernel(const float *__restrict__ w, int Cout, int Cin, int transpose,
                               const float *__restrict__ scale2, uint4 *__restrict__ out, unsigned *__restrict__ lo_flag) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int CK = Cin / 16;
    const int64_t total = (int64_t)(Cout / 32) * CK * 9 * 2 * 64;
    if (idx >= total) return;
    int64_t r = idx;
    const int lane = (int)(r % 64); r /= 64;
    const int hl = (int)(r % 2); r /= 2;
    const int kx = (int)(r % 3); r /= 3;
    const int ky = (int)(r % 3); r /= 3;
    const int ck = (int)(r % CK); r /= CK;
    const int co = (int)r * 32 + (lane & 31);
    const int kg = lane >> 5;
    const float s = scale2[0];
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = ck * 16 + kg * 8 + j;
        const int64_t src = transpose ? (((int64_t)ci * Cout + co) * 3 + (2 - ky)) * 3 + (2 - kx)
                                      : (((int64_t)co * Cin + ci) * 3 + ky) * 3 + kx;
        v[j] = w[src] * s;
    }
    uint4 hi, lo;
    split8(v, hi, lo);
    out[idx] = hl ? lo : hi;
    if (hl) note_lo(lo, lo_flag);
}

// ---- the convolution -------------------------------------------------------------------------------------
struct ConvArgs {
    const char *xs, *wp, *zero16;
    const float *bias, *chan_add, *residual, *x_scale2, *w_scale2;
    float *y;
    int N, CK, Cout, H, W, tilesX, tilesY, MB;
    // split-K (partial != nullptr): workgroup `split` of `splits` contracts channel chunks [split*cks, (split+1)*cks) and
    // writes its raw accumulators to partial[split][n][Cout][H][W]; cv_split_reduce_kernel sums them in order
    int splits, cks;
    float *partial;
    // GroupNorm moment partials of the OUTPUT from the unsplit epilogue (round 6; null = none): per (image, output channel,
    // pixel tile, wave) the fp32 sum and sum of squares of the wave's 64 finished values MINUS a shift K (one of the 64 values)
    // and K itself, tile_part[(((n * Cout + co) * tiles + tile) * 4 + wave) * 4 + {0, 1, 2}] (word 3 unused);
    // gn_moments_from_tiles_kernel restores the raw moments and adds them in fp64 in index order.  The GroupNorm
    // that reads y next then needs no pass over y for its statistics (it was gn_moments_kernel: one full read of y).
    float *tile_part;
    int prio;                    // 1: the co-resident workgroups alternate their wave priority stage by stage
#ifdef MVIP_EXPERIMENT_CONV
    int dbg;                     // timing experiments (MVIP_CONV_DBG): 1 = no epilogue, 2 = no MFMAs, 4 = no input DMA, 8 = no weight DMA, 16 = no barrier, 32 = linear B reads
    unsigned long long *probe;   // per workgroup (8 words): {shader cycles total, 100 MHz ticks total, prologue, DMA issue, compute, epilogue, barrier wait, start tick}
#endif
};

// MT <= 2: 80 KB of LDS and 256 registers, i.e. TWO workgroups per CU = two waves per SIMD, so one wave's LDS
// reads, waits and epilogue run under the other wave's MFMAs.
// TW = 32: pixel tile 8 rows x 32 columns, an MFMA column block (32 pixels) = one image row of the tile.
// TW = 16 (images narrower than 32 pixels: the UNet's 16x16 level): tile 16 x 16, a column block = two rows of 16.
// NW = 8 (TW = 32 only, opt-in): a workgroup of eight waves owns a 16 x 32 pixel tile, so the weights of a stage and
// the haloed input tile are shared by twice the MFMAs (10.9 instead of 16.8 B/clk/CU of LDS-DMA at full matrix rate for
// MT = 2).  Built to test whether operand delivery bounds this kernel as it bounds the plain GEMM and the attention
// kernel: it does not -- both shapes run the VAE / UNet convolutions in the same time (round 2, tools/conv_wide_ab.py).
// TW = 8 (8 x 8 images, the UNet's innermost level): a workgroup takes FOUR images, wave w image w (two column blocks of
// 4 rows x 8 pixels); the LDS tile holds the four haloed 10 x 10 images one after the other.
// Split-K: at the inner UNet levels the grid of (pixel tile, row block) pairs is far smaller than the chip (1280 channels
// at 16 x 16 x 2 images: 80 workgroups, at 8 x 8: 40) while one layer's weights are 59-118 MB, so those layers are bound by
// how many CUs pull weights at once; with a.partial set the channel range is divided over a.splits workgroups.
// F16 (the reference's --fp16 mode, DS_NeRF/guidance/sd_utils.py:66): ONE fp16 product per contraction step -- only the hi
// plane of the activations and the hi fragments of the weights are fetched (the lo halves of both operand images are
// neither read nor, by the producers, written), fp32 accumulation; a third of the matrix work and half the operand traffic.
// NP = 3 / 2 / 1 products per step (see the file header): 2 = the weights' lo fragments are zero and not fetched.
template <int MT, int TW = CV_TW, int NW = 4, int NP = 3>
__global__ void __launch_bounds__(NW * 64, (NW == 8 ? (MT <= 2 ? 2 : 1) : (MT <= 2 ? 2 : 1))) conv3x3_f16x3_kernel(const ConvArgs a) {
    constexpr bool F16 = NP == 1;
    constexpr int NT = NW * 64;
    constexpr int TH = NT / TW, HW = TW + 2, RPB = 32 / TW;                         // RPB: image rows per column block
    constexpr int PIX = TW == 8 ? 4 * 10 * HW : (TH + 2) * HW;
    constexpr int CV_IN_BYTES = 4 * PIX * 16;          // shadows the 8 x 32 constants: sized for this tile
    constexpr int CV_IN_ROUNDS = (4 * PIX + NT - 1) / NT;
    constexpr int WB = 3 * MT * 2 * 1024;              // weights of one stage (kernel row, 16 channels)
    __shared__ __attribute__((aligned(16))) char lds[3 * WB + 2 * CV_IN_BYTES];
    char *lds_w = lds, *lds_in = lds + 3 * WB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l32 = lane & 31, kg = lane >> 5;
#ifdef MVIP_EXPERIMENT_CONV
    unsigned long long pc0 = 0, pr0 = 0, p_sync = 0, p_comp = 0, p_pro = 0, p_mark = 0, p_bar = 0;
    if (a.probe) { pc0 = __builtin_amdgcn_s_memtime(); pr0 = __builtin_amdgcn_s_memrealtime(); }
#define CV_MARK(acc_) do { if (a.probe) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc_ += now_ - p_mark; p_mark = now_; } } while (0)
#else
#define CV_MARK(acc_) do { } while (0)
#endif
    // XCD-aware order: each of the 8 XCDs walks a contiguous range of (tile, channel-block) pairs, the
    // channel blocks of one pixel tile adjacent in time, so the tile's planes are served by that XCD's L2.
    int id = blockIdx.x;
    const int total = gridDim.x;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    const int split = id % a.splits;                    // the splits of one (tile, row block) adjacent: they share the input tile
    id /= a.splits;
    const int mb = id % a.MB;
    int tile = id / a.MB;
    const int tx = tile % a.tilesX; tile /= a.tilesX;
    const int ty = tile % a.tilesY;
    const int n = (TW == 8 ? 4 : 1) * (tile / a.tilesY);                 // first image of the workgroup
    const int y0 = ty * TH, x0 = tx * TW;
    const int H = a.H, W = a.W;
    const int64_t plane = (int64_t)H * W * 16;
    const int ck0 = split * a.cks;
    const int nck = (a.CK - ck0 < a.cks) ? a.CK - ck0 : a.cks;           // channel chunks of this workgroup (>= 1)

    int in_off[CV_IN_ROUNDS];
#pragma unroll
    for (int r = 0; r < CV_IN_ROUNDS; ++r) {
        const int s = r * NT + tid;
        in_off[r] = s < 4 * PIX ? -1 : -2;             // -1: halo outside the image (zero page), -2: no slot
        if (F16 && s < 4 * PIX && ((s / PIX) & 1)) in_off[r] = -2;        // lo planes (piece = kg*2 + hl) are not fetched
        if (s < 4 * PIX && in_off[r] != -2) {
            const int piece = s / PIX, p = s - piece * PIX;
            const int row = p / HW, col = p - row * HW;
            if constexpr (TW == 8) {
                const int img = row / 10, gy = row - img * 10 - 1, gx = col - 1;
                if (n + img < a.N && gy >= 0 && gy < 8 && gx >= 0 && gx < 8)
                    in_off[r] = (int)(img * a.CK * 4 * plane) + (int)(piece * plane) + (gy * 8 + gx) * 16;
            } else {
                const int gy = y0 - 1 + row, gx = x0 - 1 + col;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) in_off[r] = (int)(piece * plane) + (gy * W + gx) * 16;
            }
        }
    }
    const char *xs_n = a.xs + ((int64_t)n * a.CK + ck0) * 4 * plane;
    constexpr int WROW = 3 * 2 * 1024;                 // one stage of one 32-channel row block
    const char *wp_b = a.wp + ((int64_t)mb * MT * a.CK + ck0) * 3 * WROW;

    auto issue_input = [&](int ck, int buf) {
#ifdef MVIP_EXPERIMENT_CONV
        if (a.dbg & 4) return;
#endif
        const char *base = xs_n + (int64_t)ck * 4 * plane;
        char *dst = lds_in + buf * CV_IN_BYTES + wave * 1024;
#pragma unroll
        for (int r = 0; r < CV_IN_ROUNDS; ++r)
            if (in_off[r] != -2) glds16b(in_off[r] >= 0 ? base + in_off[r] : a.zero16, dst + r * (NT * 16));
    };
    auto issue_weights = [&](int t, int buf) {
#ifdef MVIP_EXPERIMENT_CONV
        if (a.dbg & 8) return;
#endif
        const char *src = wp_b + (int64_t)t * WROW + lane * 16;
        char *dst = lds_w + buf * WB;
#pragma unroll
        for (int b0 = 0; b0 < 6 * MT; b0 += NW) {       // LDS block b = m*6 + kx*2 + hl
            const int b = b0 + wave;
            if (b < 6 * MT && !(NP < 3 && (b & 1)))        // b odd = lo fragments (fetched by the three-product kernel only)
                glds16b(src + (int64_t)(b / 6) * a.CK * 3 * WROW + (b % 6) * 1024, dst + b * 1024);
        }
    };

    f32x16 acc[MT][2];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;

    // Software pipeline.  A "group" = one tap (kx) of one 32-channel output row block m: two A fragments (hi, lo),
    // the tap's four B fragments, six MFMAs on two independent accumulators.  Fragments are read from LDS TWO
    // groups ahead of their use, right after the first pair of MFMAs of a group and pinned there by scheduling
    // barriers: this kernel runs one wave per SIMD, so nothing hides an exposed LDS latency (the first version
    // read, waited and multiplied group by group and kept the matrix pipe 34 % busy).  Weights are staged TWO
    // stages ahead in three LDS buffers so that the next stage's fragments can be read before the barrier.
    constexpr int NG = 3 * MT;                          // groups per stage, kx-major
    const int nstage = nck * 3;
    const int jrow0 = 2 * wave;
    const int img_rows = TW == 8 ? 2 * wave : 0;        // TW = 8: every image in front of this wave's adds two halo rows
    // PD = groups between a fragment's LDS read and its use (NS sets of A fragments, set = group % NS, NG % NS == 0 so the
    // rotation survives stages).  Two groups; four (PD = 4, NS = 6 at MT = 2: ~770 cycles of cover, 203 registers)
    // measured the same on every VAE / UNet shape -- the LDS read latency is not what the waves wait for.
    constexpr int PD = 2;
    constexpr int NS = 3;
    h16x8 Ah[NS], Al[NS];
    h16x8 Bh[3][2], Bl[3][2];                           // set = kx: the tap PD groups ahead is always the one just finished
    auto load_a = [&](const char *wb, int g, int set) {
        const int kx = g / MT, m = g % MT;
        Ah[set] = *reinterpret_cast<const h16x8 *>(wb + ((m * 3 + kx) * 2 + 0) * 1024);
        if constexpr (NP == 3) Al[set] = *reinterpret_cast<const h16x8 *>(wb + ((m * 3 + kx) * 2 + 1) * 1024);
    };
    auto load_b = [&](const char *inb, int ky, int kx) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int p = ((jrow0 + j) * RPB + img_rows + l32 / TW + ky) * HW + l32 % TW + kx;
#ifdef MVIP_EXPERIMENT_CONV
            if (a.dbg & 32) p = (j * 3 + kx) * 64 + lane - (kg * 2) * PIX;          // timing only: wave-linear 1-KB fragment reads
#endif
            Bh[kx][j] = *reinterpret_cast<const h16x8 *>(inb + p * 16);
            if constexpr (!F16) Bl[kx][j] = *reinterpret_cast<const h16x8 *>(inb + PIX * 16 + p * 16);
        }
    };
    auto w_base = [&](int t) { return lds_w + (t % 3) * WB + lane * 16; };
    auto in_base = [&](int t) { return lds_in + ((t / 3) & 1) * CV_IN_BYTES + (kg * 2) * (PIX * 16); };

    issue_input(0, 0);
    issue_weights(0, 0);
    if (nstage > 1) issue_weights(1, 1);
    __syncthreads();                                    // stages 0 and 1 (and input chunk 0) have landed
    if (nstage > 2) issue_weights(2, 2);
    if (nck > 1) issue_input(1, 1);
#pragma unroll
    for (int g = 0; g < PD; ++g) {                      // PD < NG: the first PD groups are all of stage 0
        load_a(w_base(0), g, g % NS);
        if (g % MT == 0) load_b(in_base(0), 0, g / MT);
    }
#ifdef MVIP_EXPERIMENT_CONV
    if (a.probe) { p_mark = __builtin_amdgcn_s_memtime(); p_pro = p_mark - pc0; }
#endif
    // The two workgroups that share a CU sit in hardware wave slots 0 and 1 of each SIMD, and at equal priority the
    // arbiter serves the older slot first: the slot-0 workgroup of a one-round launch finished in 203 us, its partner in
    // 238 us (tools/conv_stragglers.py), the last 35 us with one wave per SIMD.  Alternating the priority stage by stage
    // (s_setprio; MVIP_CONV_PRIO=1) makes the pair finish together (226 / 232 us) and the launch 3 % shorter, which the
    // whole SDS step does not show (9.95 vs 10.0 ms of convolutions) -- off by default.
    const int prio_phase = a.prio ? (int)(__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 4) & 1u) : -1;
    for (int t = 0; t < nstage; ++t) {
        const int ck = t / 3, ky = t - ck * 3;
        if (prio_phase >= 0) { if ((t + prio_phase) & 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
        CV_MARK(p_comp);
        if (t > 0) {
#ifdef MVIP_EXPERIMENT_CONV
            if (!(a.dbg & 16))
#endif
            __syncthreads();                   // stage t+1 landed (vmcnt(0)); every wave is done with stage t-1
            CV_MARK(p_bar);
            if (t + 2 < nstage) issue_weights(t + 2, (t + 2) % 3);
            if (ky == 0 && ck + 1 < nck) issue_input(ck + 1, (ck + 1) & 1);
        }
        CV_MARK(p_sync);
        const char *wb = w_base(t), *inb = in_base(t);
        const char *wb_n = w_base(t + 1), *inb_n = in_base(t + 1);
        const int ky_n = (ky == 2) ? 0 : ky + 1;
        const bool more = t + 1 < nstage;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int kx = g / MT, m = g % MT, set = g % NS;
#ifdef MVIP_EXPERIMENT_CONV
            if (a.dbg & 2) {
                acc[m][0][0] += (float)Ah[set][0] + (float)Bh[kx][0][0] + (float)Bl[kx][1][0];
                acc[m][1][0] += (float)Al[set][0] + (float)Bh[kx][1][0] + (float)Bl[kx][0][0];
                const int g2 = g + PD;
                if (g2 < NG) { load_a(wb, g2, g2 % NS); if (g2 % MT == 0) load_b(inb, ky, g2 / MT); }
                else if (more) { load_a(wb_n, g2 - NG, g2 % NS); if ((g2 - NG) % MT == 0) load_b(inb_n, ky_n, (g2 - NG) / MT); }
                continue;
            }
#endif
            acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[set], Bh[kx][0], acc[m][0], 0, 0, 0);
            acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[set], Bh[kx][1], acc[m][1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            {   // fragments of group g+PD (this stage or the next one)
                const int g2 = g + PD;
                if (g2 < NG) {
                    load_a(wb, g2, g2 % NS);
                    if (g2 % MT == 0) load_b(inb, ky, g2 / MT);
                } else if (more) {
                    load_a(wb_n, g2 - NG, g2 % NS);
                    if ((g2 - NG) % MT == 0) load_b(inb_n, ky_n, (g2 - NG) / MT);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NP >= 2) {
                acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[set], Bl[kx][0], acc[m][0], 0, 0, 0);
                acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[set], Bl[kx][1], acc[m][1], 0, 0, 0);
            }
            if constexpr (NP == 3) {               // NP == 2: Al == 0 -- this pair would add exact zeros
                acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al[set], Bh[kx][0], acc[m][0], 0, 0, 0);
                acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al[set], Bh[kx][1], acc[m][1], 0, 0, 0);
            }
        }
    }

    CV_MARK(p_comp);
    const float inv = a.w_scale2[1] * (a.x_scale2 ? a.x_scale2[1] : 1.f);
    const int gx = x0 + l32 % TW;
    const int n_out = TW == 8 ? n + wave : n;
    if (TW == 8 && n_out >= a.N) return;
#ifdef MVIP_EXPERIMENT_CONV
    if (a.dbg & 1) {
        float t = 0.f;
        for (int m = 0; m < MT; ++m) for (int j = 0; j < 2; ++j) for (int r = 0; r < 16; ++r) t += acc[m][j][r];
        if (t == 123.456f) a.y[0] = t;
        if (a.probe && tid == 0) {
            const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
            unsigned long long *o = a.probe + 8 * (unsigned long long)blockIdx.x;
            o[0] = c1 - pc0; o[1] = r1 - pr0; o[2] = p_pro; o[3] = p_sync; o[4] = p_comp; o[5] = c1 - p_mark; o[6] = p_bar; o[7] = pr0;
        }
        return;
    }
#endif
    // The epilogue's loads are issued TOGETHER, ahead of the arithmetic: written element by element (`if (bias) v +=
    // bias[co]; if (chan_add) ...; if (residual) v += residual[o]; y[o] = v`) every load sits behind its own branch and
    // is followed by s_waitcnt vmcnt(0) -- up to 3 x 64 exposed memory latencies per wave, 122 k of the 211 k cycles of a
    // 128-channel 512 x 512 workgroup (tools/conv_probe.py).
    auto out_index = [&](int m, int j, int r, int &co) -> int64_t {
        const int gy = TW == 8 ? j * RPB + l32 / TW : y0 + (jrow0 + j) * RPB + l32 / TW;
        co = (mb * MT + m) * 32 + 8 * (r >> 2) + 4 * kg + (r & 3);
        return (((int64_t)n_out * a.Cout + co) * H + gy) * W + gx;
    };
    if (a.partial) {
        float *pp = a.partial + (int64_t)split * a.N * a.Cout * H * W;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { int co; pp[out_index(m, j, r, co)] = acc[m][j][r]; }
    } else {
        const bool hb = a.bias != nullptr, hc = a.chan_add != nullptr, hr = a.residual != nullptr;
        float bv[MT][16], cv[MT][16];
        f32x16 rv[MT][2];
        if (hr) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { int co; rv[m][j][r] = a.residual[out_index(m, j, r, co)]; }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (mb * MT + m) * 32 + 8 * (r >> 2) + 4 * kg + (r & 3);
                bv[m][r] = hb ? a.bias[co] : 0.f;
                cv[m][r] = hc ? a.chan_add[(int64_t)n_out * a.Cout + co] : 0.f;
            }
        bool with_moments = false;
        if constexpr (TW != 8 && NW == 4) with_moments = a.tile_part != nullptr;
        if (!with_moments) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        int co;
                        const int64_t o = out_index(m, j, r, co);
                        float v = acc[m][j][r] * inv;
                        if (hb) v += bv[m][r];
                        if (hc) v += cv[m][r];
                        if (hr) v += rv[m][j][r];
                        a.y[o] = v;
                    }
        }
        if constexpr (TW != 8 && NW == 4) {
            if (with_moments) {
                // The same stores, channel by channel (both pixels of a register pair finished together), and the channel's
                // moment partial right behind them.  Register r of lane (l32, kg) holds output channel 8 (r >> 2) + 4 kg + (r & 3)
                // of row tile m at the two pixels (j = 0, 1) of column l32: the channel's sum over the wave's 64 pixels = the two
                // values added, then the total over the 32 lanes of the half-wave -- four row_shr steps (lane 15 of each 16-lane
                // row = the row's total) and one row_bcast:15 into rows 1 and 3 (lanes 31 / 63 = the half-waves' totals).  Five
                // DPP adds per statistic and channel on the VALU, under the co-resident workgroup's MFMAs; no LDS, no barrier.
                const int tiles = a.tilesX * a.tilesY, tile_lin = ty * a.tilesX + tx;
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        int co;
                        const int64_t o0 = out_index(m, 0, r, co), o1 = out_index(m, 1, r, co);
                        float v0 = acc[m][0][r] * inv, v1 = acc[m][1][r] * inv;
                        if (hb) { v0 += bv[m][r]; v1 += bv[m][r]; }
                        if (hc) { v0 += cv[m][r]; v1 += cv[m][r]; }
                        if (hr) { v0 += rv[m][0][r]; v1 += rv[m][1][r]; }
                        a.y[o0] = v0;
                        a.y[o1] = v1;
                        // Moments about a shift K, the channel's value at the half-wave's first pixel: E[y^2] - mean^2 of a row whose
                        // mean is 100 standard deviations (residual streams) loses the variance to the fp32 rounding of the raw
                        // squares (relative error (mean / std)^2 ulps); the deviations from a value of the row itself are of the
                        // order of the standard deviation, and the reduction restores the raw moments in fp64.
                        const float k_lo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v0), 0));
                        const float k_hi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v0), 32));
                        const float K = kg ? k_hi : k_lo;
                        const float d0 = v0 - K, d1 = v1 - K;
                        float sm = d0 + d1, q = d0 * d0 + d1 * d1;
                        sm += dpp_f32<0x111>(0.f, sm); q += dpp_f32<0x111>(0.f, q);
                        sm += dpp_f32<0x112>(0.f, sm); q += dpp_f32<0x112>(0.f, q);
                        sm += dpp_f32<0x114>(0.f, sm); q += dpp_f32<0x114>(0.f, q);
                        sm += dpp_f32<0x118>(0.f, sm); q += dpp_f32<0x118>(0.f, q);
                        sm += dpp_f32<0x142, 0xa>(0.f, sm); q += dpp_f32<0x142, 0xa>(0.f, q);
                        if (l32 == 31) {
                            float4 *dst = reinterpret_cast<float4 *>(a.tile_part) + (((int64_t)n_out * a.Cout + co) * tiles + tile_lin) * 4 + wave;
                            *dst = make_float4(sm, q, K, 0.f);
                        }
                    }
            }
        }
    }
#ifdef MVIP_EXPERIMENT_CONV
    if (a.probe && tid == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        unsigned long long *o = a.probe + 8 * (unsigned long long)blockIdx.x;
        o[0] = c1 - pc0; o[1] = r1 - pr0; o[2] = p_pro; o[3] = p_sync; o[4] = p_comp; o[5] = c1 - p_mark; o[6] = p_bar; o[7] = pr0;
        if (a.dbg & 64) o[5] = __builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) << 32);   // HW_ID, XCC_ID
    }
#endif
}

// y = (sum_s partial[s]) / (s_w s_x) + bias + chan_add + residual, the splits added in index order (deterministic)
__global__ void cv_split_reduce_kernel(const float *__restrict__ partial, int splits, int64_t total, int Cout, int64_t HW,
                                       const float *__restrict__ w_scale2, const float *__restrict__ x_scale2,
                                       const float *__restrict__ bias, const float *__restrict__ chan_add,
                                       const float *__restrict__ residual, float *__restrict__ y) {
    // grid (ceil(HW / 1024), N * Cout): the row (n, co) is the block's y index -- a flat 64-bit index cost two 64-bit
    // divisions per thread, as much time as the memory traffic of these small tensors
    const int64_t p4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;        // HW % 4 == 0: four pixels of one channel
    if (p4 >= HW) return;
    const float inv = w_scale2[1] * (x_scale2 ? x_scale2[1] : 1.f);
    const unsigned rows = (unsigned)(total / HW);      // wave-uniform; N * Cout < 2^31
  for (unsigned nc = blockIdx.y; nc < rows; nc += gridDim.y) {                      // n * Cout + co (one trip unless rows > 65535)
    const int64_t i4 = (int64_t)nc * HW + p4;
    f32x4 sum = *reinterpret_cast<const f32x4 *>(partial + i4);
    int s = 1;
    for (; s + 3 < splits; s += 4) {                   // four loads in flight, added in index order
        const f32x4 p0 = *reinterpret_cast<const f32x4 *>(partial + (int64_t)s * total + i4);
        const f32x4 p1 = *reinterpret_cast<const f32x4 *>(partial + (int64_t)(s + 1) * total + i4);
        const f32x4 p2 = *reinterpret_cast<const f32x4 *>(partial + (int64_t)(s + 2) * total + i4);
        const f32x4 p3 = *reinterpret_cast<const f32x4 *>(partial + (int64_t)(s + 3) * total + i4);
        sum += p0; sum += p1; sum += p2; sum += p3;
    }
    for (; s < splits; ++s) sum += *reinterpret_cast<const f32x4 *>(partial + (int64_t)s * total + i4);
    f32x4 v = sum * inv;                               // same order of roundings as the unsplit epilogue
    if (bias) v += bias[nc % (unsigned)Cout];
    if (chan_add) v += chan_add[nc];
    if (residual) v += *reinterpret_cast<const f32x4 *>(residual + i4);
    *reinterpret_cast<f32x4 *>(y + i4) = v;
  }
}

// The same reduction that also leaves the GroupNorm moments of its OUTPUT rows, in the layout gn_moments_kernel
// (csrc/group_norm.hip) writes for HW <= 4096 (one {sum, sum of squares} fp64 pair per (sample, channel) row): the next
// layer's GroupNorm then needs no pass over y for its statistics.  A row (HW = 64, 256, 1024 or 4096 values) is owned by
// LPR = min(HW / 4, 256) consecutive threads (rows of 1024+ values: one workgroup, looping), so the sums are formed in a
// fixed order: per thread in index order, a DPP scan over the row's lanes, then the four waves in order.
template <int LPR, int IT = 1>
__global__ void __launch_bounds__(256)
cv_split_reduce_moments_kernel(const float *__restrict__ partial, int splits, int64_t total, int Cout, int64_t HW,
                               const float *__restrict__ w_scale2, const float *__restrict__ x_scale2,
                               const float *__restrict__ bias, const float *__restrict__ chan_add,
                               const float *__restrict__ residual, float *__restrict__ y, double *__restrict__ moments) {
    constexpr int ROWS = 256 / LPR;                           // rows per workgroup
    const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / LPR;             // n * Cout + co
    const int lr = threadIdx.x % LPR;
    const float inv = w_scale2[1] * (x_scale2 ? x_scale2[1] : 1.f);
    const float bv = bias ? bias[(unsigned)row % (unsigned)Cout] : 0.f, cv = chan_add ? chan_add[row] : 0.f;      // N * Cout < 2^31
    double sm = 0.0, q = 0.0;
    const int64_t i0 = row * HW + (int64_t)lr * 4;        // IT pieces of LPR * 4 values per row, all loads of a split in flight
    f32x4 sum[IT], rv[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        sum[it] = *reinterpret_cast<const f32x4 *>(partial + i0 + (int64_t)it * LPR * 4);
        if (residual) rv[it] = *reinterpret_cast<const f32x4 *>(residual + i0 + (int64_t)it * LPR * 4);
    }
    for (int sp = 1; sp < splits; ++sp) {
        f32x4 t[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) t[it] = *reinterpret_cast<const f32x4 *>(partial + (int64_t)sp * total + i0 + (int64_t)it * LPR * 4);
#pragma unroll
        for (int it = 0; it < IT; ++it) sum[it] += t[it];
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        f32x4 v = sum[it] * inv;                           // same order of roundings as cv_split_reduce_kernel
        if (bias) v += bv;
        if (chan_add) v += cv;
        if (residual) v += rv[it];
        *reinterpret_cast<f32x4 *>(y + i0 + (int64_t)it * LPR * 4) = v;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const double d = (double)v[k]; sm += d; q += d * d; }
    }
    // totals over the row's lanes on DPP row operations (common.h; a dozen VALU steps instead of 24 dependent ds_bpermute round
    // trips): the four row_shr steps leave a 16-lane row's total in its last lane, the two broadcasts the wave's in lane 63
    sm += dpp_f64<0x111>(0.0, sm); q += dpp_f64<0x111>(0.0, q);
    sm += dpp_f64<0x112>(0.0, sm); q += dpp_f64<0x112>(0.0, q);
    sm += dpp_f64<0x114>(0.0, sm); q += dpp_f64<0x114>(0.0, q);
    sm += dpp_f64<0x118>(0.0, sm); q += dpp_f64<0x118>(0.0, q);
    if constexpr (LPR >= 64) {
        sm += dpp_f64<0x142, 0xa>(0.0, sm); q += dpp_f64<0x142, 0xa>(0.0, q);
        sm += dpp_f64<0x143, 0xc>(0.0, sm); q += dpp_f64<0x143, 0xc>(0.0, q);
    }
    if constexpr (LPR == 256) {
        __shared__ double red[2][4];
        if ((threadIdx.x & 63) == 63) { red[0][threadIdx.x >> 6] = sm; red[1][threadIdx.x >> 6] = q; }
        __syncthreads();
        sm = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        q = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
    if (lr == LPR - 1) { moments[row * 2] = sm; moments[row * 2 + 1] = q; }
}

// GroupNorm moments of a convolution output from the tile partials its unsplit epilogue left (ConvArgs::tile_part): each
// partial (s, q, K) holds the fp32 sum and sum of squares of 64 values about the shift K, i.e. raw moments s + 64 K and
// q + 2 K s + 64 K^2, formed here in fp64; the (image, channel) row's `parts` of them added in fp64 and written in the layout
// gn_moments_kernel leaves for this row length (`chunks` pairs per row: the total in the first, zeros in the rest), which is
// what cv_to_split_kernel<GN> and gn_finalize_kernel read.
__device__ __forceinline__ void tile_partial_add(const float4 t, double &sm, double &q) {
    const double s = (double)t.x, k = (double)t.z;
    sm += s + 64.0 * k;
    q += (double)t.y + k * (2.0 * s + 64.0 * k);
}

__global__ void __launch_bounds__(256)
gn_moments_from_tiles_kernel(const float4 *__restrict__ part, int parts, int64_t rows, int chunks, double *__restrict__ out) {
    // one WORKGROUP per row (the first version -- one wave per row, one load in flight per lane -- took 17.6 us per launch at
    // 4,096 partials per row: as long as the pass over y it replaces): thread t adds partials t, t + 256, ... four loads in
    // flight, then the xor tree inside each wave and the four waves in index order -- a fixed order, bit-reproducible
    __shared__ double red[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = blockIdx.x;
    const float4 *p = part + row * parts;
    double sm = 0.0, q = 0.0;
    int i = threadIdx.x;
    for (; i + 768 < parts; i += 1024) {
        const float4 t0 = p[i], t1 = p[i + 256], t2 = p[i + 512], t3 = p[i + 768];
        tile_partial_add(t0, sm, q); tile_partial_add(t1, sm, q); tile_partial_add(t2, sm, q); tile_partial_add(t3, sm, q);
    }
    for (; i < parts; i += 256) tile_partial_add(p[i], sm, q);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 64); q += __shfl_xor(q, o, 64); }
    if (lane == 0) { red[0][wave] = sm; red[1][wave] = q; }
    __syncthreads();
    if (threadIdx.x < chunks) {
        const double ts = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3], tq = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        out[(row * chunks + threadIdx.x) * 2] = threadIdx.x == 0 ? ts : 0.0;
        out[(row * chunks + threadIdx.x) * 2 + 1] = threadIdx.x == 0 ? tq : 0.0;
    }
}

}  // namespace mvip

using namespace mvip;

void mvip::launch_split_reduce(const float *partial, int splits, int64_t rows, int M, int64_t HW, const float *w_scale2,
                               const float *x_scale2, const float *bias, const float *chan_add, const float *residual,
                               float *y, hipStream_t st) {
    hipLaunchKernelGGL(cv_split_reduce_kernel, dim3((unsigned)((HW / 4 + 255) / 256), (unsigned)(rows > 65535 ? 65535 : rows)), dim3(256), 0, st,
                       partial, splits, rows * HW, M, HW, w_scale2, x_scale2, bias, chan_add, residual, y);
}

extern "C" int mvip_conv3x3_supported(int64_t Cout, int64_t Cin, int64_t H, int64_t W) {
    return Cout > 0 && Cout % 32 == 0 && Cin > 0 && Cin % 16 == 0 && H > 0 && W > 0 &&
           ((H % CV_TH == 0 && W % CV_TW == 0) || (H % 16 == 0 && W % 16 == 0) || (H == 8 && W == 8)) &&
           H * W <= (1 << 24);
}

extern "C" int64_t mvip_conv3x3_packed_bytes(int64_t Cout, int64_t Cin) {
    if (Cout <= 0 || Cin <= 0) return 0;
    return Cout * Cin * 9 * 4 + 256;       // tail: {scale, 1/scale, absmax bits}, then a 16-byte zero page
}

// tail layout (byte offsets from Cout*Cin*36): 0 scale, 4 1/scale, 8 absmax bits, 12 "a lo fragment is non-zero", 128..143 zeros
extern "C" int mvip_conv3x3_pack(const float *weight, int64_t Cout, int64_t Cin, int transpose, void *packed,
                                 void *stream) {
    const int64_t co = transpose ? Cin : Cout, ci = transpose ? Cout : Cin;      // operator dims
    if (!weight || !packed || co <= 0 || co % 32 != 0 || ci <= 0 || ci % 16 != 0) return MVIP_EINVAL;
    hipStream_t st = as_stream(stream);
    char *tail = (char *)packed + co * ci * 36;
    zero_words(tail, 64, st);
    launch_absmax_then_scale(weight, Cout * Cin * 9, (unsigned *)(tail + 8), (float *)tail, st);
    const int64_t total = (co / 32) * (ci / 16) * 9 * 2 * 64;
    hipLaunchKernelGGL(cv_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, weight, (int)co, (int)ci,
                       transpose, (const float *)tail, (uint4 *)packed, (unsigned *)(tail + 12));
    return check_launch();
}

// Number of channel splits for a launch whose unsplit grid has `blocks` workgroups: fill ~2 workgroups per CU, keep at
// least 4 channel chunks (12 stages) per workgroup so the pipeline prologue stays small.
static inline int cv_splits(int64_t blocks, int64_t CK) {
    static const int forced = [] { const char *e = getenv("MVIP_CONV_SPLITS"); return e ? atoi(e) : 0; }();   // tuning
    // the chip holds 512 of these workgroups at a time: as many splits as keep the launch within ONE round (the probe of
    // tools/conv_probe.py on 640 channels at 32 x 32: 560 workgroups = 1.09 rounds took 72 us, the median workgroup 42)
    int64_t s = forced > 0 ? forced : (blocks >= 256 ? 1 : 512 / blocks);
    if (s > CK / 4) s = CK / 4;
    if (s > 32) s = 32;
    if (s < 1) s = 1;
    const int64_t cks = (CK + s - 1) / s;
    return (int)((CK + cks - 1) / cks);                // no empty split
}
static inline void cv_geometry(int64_t N, int64_t Cout, int64_t H, int64_t W, int &tw, int &MT, int64_t &blocks) {
    tw = (W % CV_TW == 0 && H % CV_TH == 0) ? CV_TW : (H == 8 && W == 8 ? 8 : 16);
    const int th = 256 / tw;
    MT = tw != CV_TW ? 1 : cv_mt(Cout, N * (W / tw) * (H / th));
    // 64-row workgroups also on small grids (the fragment reads and the input DMA of a stage serve twice the MFMAs); the
    // channel splits fill the chip instead of the row blocks: 12.0 -> 11.3 ms of convolutions per SDS step, +0.3 ms of
    // split reduction.  MVIP_CONV_MT2=0 restores the 32-row choice (A-B switch).
    static const int mt2_env = [] { const char *e = getenv("MVIP_CONV_MT2"); return e ? atoi(e) : 1; }();
    if (mt2_env && tw == CV_TW && MT == 1 && Cout % 64 == 0) MT = 2;
    blocks = (tw == 8 ? (N + 3) / 4 : N * (W / tw) * (H / th)) * (Cout / (32 * MT));
}

extern "C" int64_t mvip_conv3x3_workspace_bytes(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W) {
    if (N <= 0 || !mvip_conv3x3_supported(Cout, Cin, H, W)) return 0;
    int tw, MT;
    int64_t blocks;
    cv_geometry(N, Cout, H, W, tw, MT, blocks);
    const int s = cv_splits(blocks, Cin / 16);
    return s > 1 ? (int64_t)s * N * Cout * H * W * 4 : 0;
}

static int conv3x3_launch(const void *xs, const void *packed, const float *bias, const float *chan_add,
                          const float *residual, const float *x_scale2, int64_t N, int64_t Cin, int64_t Cout,
                          int64_t H, int64_t W, float *y, void *workspace, int prec, void *stream,
                          double *row_moments = nullptr, float *tile_part = nullptr) {
    if (N < 0 || !mvip_conv3x3_supported(Cout, Cin, H, W) || prec < 0 || prec > 2) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!xs || !packed || !y) return MVIP_EINVAL;
    int tw, MT;
    int64_t blocks;
    cv_geometry(N, Cout, H, W, tw, MT, blocks);
    const int th = 256 / tw;
    ConvArgs a;
    a.xs = (const char *)xs; a.wp = (const char *)packed;
    const char *tail = (const char *)packed + Cout * Cin * 36;
    a.w_scale2 = (const float *)tail; a.zero16 = tail + 128;
    a.bias = bias; a.chan_add = chan_add; a.residual = residual; a.x_scale2 = x_scale2; a.y = y;
    a.N = (int)N; a.CK = (int)(Cin / 16); a.Cout = (int)Cout; a.H = (int)H; a.W = (int)W;
    a.tilesX = (int)(W / tw); a.tilesY = (int)(H / th); a.MB = (int)(Cout / (32 * MT));
    if (tw == 8) { a.tilesX = 1; a.tilesY = 1; }
    a.splits = 1; a.cks = a.CK; a.partial = nullptr; a.tile_part = nullptr;
    { static const int pr = [] { const char *e = getenv("MVIP_CONV_PRIO"); return e ? atoi(e) : 0; }(); a.prio = pr; }
#ifdef MVIP_EXPERIMENT_CONV
    { const char *e = getenv("MVIP_CONV_DBG"); a.dbg = e ? atoi(e) : 0; }
    { const char *e = getenv("MVIP_CONV_PROBE"); a.probe = e ? (unsigned long long *)strtoull(e, nullptr, 0) : nullptr; }
#endif
    hipStream_t st = as_stream(stream);
    // eight-wave workgroups on 16 x 32 pixel tiles (MVIP_CONV_WIDE=1; tuning switch, default off: measured equal to the
    // four-wave tile on every VAE / UNet shape and on the whole step, 7.56 vs 7.65 ms -- tools/conv_wide_ab.py)
    static const int wide_mode = [] { const char *e = getenv("MVIP_CONV_WIDE"); return e ? atoi(e) : 0; }();
    if (tw == CV_TW && wide_mode && H % 16 == 0 && prec != 1) {
        const int64_t tiles16 = N * (W / CV_TW) * (H / 16);
        int mtw = (Cout % 64 == 0 && tiles16 * (Cout / 64) >= 256) ? 2 : (tiles16 * (Cout / 32) >= 256 ? 1 : 0);
        // (MVIP_CONV_WIDE=2 -- 128 rows x 512 pixels per eight-wave workgroup, 12 fragment reads per 24 MFMAs instead of 16 --
        //  was measured no faster in round 3 and its <4, 32, 8, 3> instantiation spilled 164 registers: removed in round 5.)
        if (mtw) {
            a.tilesY = (int)(H / 16); a.MB = (int)(Cout / (32 * mtw));
            const int64_t wb = tiles16 * a.MB;
            if (wb > 0x7fffffffLL) return MVIP_EINVAL;
            if (mtw == 2 && prec == 2)
                hipLaunchKernelGGL((conv3x3_f16x3_kernel<2, CV_TW, 8, 2>), dim3((unsigned)wb), dim3(512), 0, st, a);
            else if (mtw == 2)
                hipLaunchKernelGGL((conv3x3_f16x3_kernel<2, CV_TW, 8>), dim3((unsigned)wb), dim3(512), 0, st, a);
            else if (prec == 2)
                hipLaunchKernelGGL((conv3x3_f16x3_kernel<1, CV_TW, 8, 2>), dim3((unsigned)wb), dim3(512), 0, st, a);
            else
                hipLaunchKernelGGL((conv3x3_f16x3_kernel<1, CV_TW, 8>), dim3((unsigned)wb), dim3(512), 0, st, a);
            return check_launch();
        }
    }
    if (workspace) {
        a.splits = cv_splits(blocks, a.CK);
        if (a.splits > 1) { a.cks = (a.CK + a.splits - 1) / a.splits; a.partial = (float *)workspace; }
    }
    blocks *= a.splits;
    if (blocks > 0x7fffffffLL) return MVIP_EINVAL;
    if (tile_part) {                                           // callers ask mvip_conv3x3_tile_moments_scratch_bytes first
        if (a.partial || tw == 8 || !row_moments) return MVIP_EINVAL;
        a.tile_part = tile_part;
    }
#define MVIP_CV_LAUNCH(F16_)   /* F16_ = NP: products per step */                                                                                             \
    do {                                                                                                                      \
        if (tw == 8) hipLaunchKernelGGL((conv3x3_f16x3_kernel<1, 8, 4, F16_>), dim3((unsigned)blocks), dim3(256), 0, st, a);         \
        else if (tw == 16) hipLaunchKernelGGL((conv3x3_f16x3_kernel<1, 16, 4, F16_>), dim3((unsigned)blocks), dim3(256), 0, st, a);  \
        else if (MT == 4) hipLaunchKernelGGL((conv3x3_f16x3_kernel<4, CV_TW, 4, F16_>), dim3((unsigned)blocks), dim3(256), 0, st, a); \
        else if (MT == 2) hipLaunchKernelGGL((conv3x3_f16x3_kernel<2, CV_TW, 4, F16_>), dim3((unsigned)blocks), dim3(256), 0, st, a); \
        else hipLaunchKernelGGL((conv3x3_f16x3_kernel<1, CV_TW, 4, F16_>), dim3((unsigned)blocks), dim3(256), 0, st, a);             \
    } while (0)
    if (prec == 1) MVIP_CV_LAUNCH(1); else if (prec == 2) MVIP_CV_LAUNCH(2); else MVIP_CV_LAUNCH(3);
#undef MVIP_CV_LAUNCH
    if (tile_part) {
        const int64_t HW = H * W, rows = N * Cout;
        const int chunks = (int)(mvip_groupnorm_workspace_bytes(1, 1, HW) / 16);
        hipLaunchKernelGGL(gn_moments_from_tiles_kernel, dim3((unsigned)rows), dim3(256), 0, st, (const float4 *)tile_part,
                           a.tilesX * a.tilesY * 4, rows, chunks, row_moments);
        return check_launch();
    }
    if (row_moments && !a.partial) return MVIP_EINVAL;         // callers ask mvip_conv3x3_row_moments_doubles first
    if (a.partial) {
        const int64_t total = N * Cout * H * W, HW = H * W;
        if (row_moments) {
#define MVIP_RM(LPR_, IT_) hipLaunchKernelGGL((cv_split_reduce_moments_kernel<LPR_, IT_>), dim3((unsigned)(N * Cout / (256 / LPR_))), \
                                              dim3(256), 0, st, a.partial, a.splits, total, (int)Cout, HW, a.w_scale2, x_scale2, \
                                              bias, chan_add, residual, y, row_moments)
            if (HW == 64) MVIP_RM(16, 1); else if (HW == 256) MVIP_RM(64, 1); else if (HW == 1024) MVIP_RM(256, 1); else MVIP_RM(256, 4);
#undef MVIP_RM
        } else {
            launch_split_reduce(a.partial, a.splits, N * Cout, (int)Cout, HW, a.w_scale2, x_scale2, bias, chan_add, residual, y, st);
        }
    }
    return check_launch();
}

// Doubles of `row_moments` ([N][Cout][2]) when this shape's launch is channel-split AND its rows fit the one-pair-per-row
// layout of mvip_groupnorm_stats (H * W = 64, 256, 1024 or 4096; N * Cout a multiple of 16), else 0.
extern "C" int64_t mvip_conv3x3_row_moments_doubles(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W) {
    if (mvip_conv3x3_workspace_bytes(N, Cin, Cout, H, W) == 0) return 0;
    const int64_t HW = H * W;
    if (!(HW == 64 || HW == 256 || HW == 1024 || HW == 4096) || (N * Cout) % 16 != 0) return 0;
    if (mvip_groupnorm_workspace_bytes(1, 1, HW) != 16) return 0;              // one moment pair per row in that layout
    return N * Cout * 2;
}

extern "C" int mvip_conv3x3_f16x3_ws_moments(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                             const float *residual, const float *x_scale2, int64_t N, int64_t Cin,
                                             int64_t Cout, int64_t H, int64_t W, float *y, void *workspace, void *row_moments,
                                             int prec, void *stream) {
    if (!workspace || !row_moments || mvip_conv3x3_row_moments_doubles(N, Cin, Cout, H, W) == 0) return MVIP_EINVAL;
    return conv3x3_launch(xs, packed, bias, chan_add, residual, x_scale2, N, Cin, Cout, H, W, y, workspace, prec, stream,
                          (double *)row_moments);
}

// Bytes of `tile_scratch` for mvip_conv3x3_f16x3_tile_moments, or 0 when this shape's launch cannot leave moment partials from
// its epilogue: channel-split launches (they have mvip_conv3x3_f16x3_ws_moments), the 8 x 8 level, the eight-wave tiles.
extern "C" int64_t mvip_conv3x3_tile_moments_scratch_bytes(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W) {
    if (N <= 0 || !mvip_conv3x3_supported(Cout, Cin, H, W)) return 0;
    if (mvip_conv3x3_workspace_bytes(N, Cin, Cout, H, W) != 0) return 0;
    static const int wide_mode = [] { const char *e = getenv("MVIP_CONV_WIDE"); return e ? atoi(e) : 0; }();
    if (wide_mode) return 0;
    int tw, MT;
    int64_t blocks;
    cv_geometry(N, Cout, H, W, tw, MT, blocks);
    if (tw == 8) return 0;
    const int th = 256 / tw;
    return N * Cout * (W / tw) * (H / th) * 4 * 4 * (int64_t)sizeof(float);      // (sum, sum of squares, shift, -) per wave
}

// The unsplit convolution that ALSO leaves the GroupNorm moments of y (the statistics pass of the GroupNorm that reads y next:
// norm2 after conv1, the next block's norm1 after conv2 -- the resnet chains of the VAE encoder and the UNet,
// DS_NeRF/guidance/sd_utils.py:330-352, :390-403): moments = [N][Cout][chunks][2] fp64 in the layout of mvip_groupnorm_stats'
// workspace (mvip_groupnorm_workspace_bytes(N, Cout, H * W) bytes), what mvip_groupnorm_split_planes_moments reads.  Two
// launches (the convolution; a reduction of N * Cout rows of tile partials) instead of convolution + a full read of y.
extern "C" int mvip_conv3x3_f16x3_tile_moments(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                               const float *residual, const float *x_scale2, int64_t N, int64_t Cin,
                                               int64_t Cout, int64_t H, int64_t W, float *y, void *tile_scratch, void *moments,
                                               int prec, void *stream) {
    if (!tile_scratch || !moments || mvip_conv3x3_tile_moments_scratch_bytes(N, Cin, Cout, H, W) == 0) return MVIP_EINVAL;
    return conv3x3_launch(xs, packed, bias, chan_add, residual, x_scale2, N, Cin, Cout, H, W, y, nullptr, prec, stream,
                          (double *)moments, (float *)tile_scratch);
}

extern "C" int mvip_conv3x3_f16x3(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                  const float *residual, const float *x_scale2, int64_t N, int64_t Cin, int64_t Cout,
                                  int64_t H, int64_t W, float *y, int prec, void *stream) {
    return conv3x3_launch(xs, packed, bias, chan_add, residual, x_scale2, N, Cin, Cout, H, W, y, nullptr, prec, stream);
}

// The same with a caller-owned workspace of mvip_conv3x3_workspace_bytes(...) bytes (may be null when that is 0): layers
// whose grid would leave most of the chip idle are split over the input channels and summed by a second launch.
extern "C" int mvip_conv3x3_f16x3_ws(const void *xs, const void *packed, const float *bias, const float *chan_add,
                                     const float *residual, const float *x_scale2, int64_t N, int64_t Cin, int64_t Cout,
                                     int64_t H, int64_t W, float *y, void *workspace, int prec, void *stream) {
    if (!workspace && mvip_conv3x3_workspace_bytes(N, Cin, Cout, H, W) > 0) return MVIP_EINVAL;
    return conv3x3_launch(xs, packed, bias, chan_add, residual, x_scale2, N, Cin, Cout, H, W, y, workspace, prec, stream);
}
