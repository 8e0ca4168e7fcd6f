// Structural similarity (SSIM, Wang et al. 2004) of image batches with its gradient (beyond the reference, whose
// DS_NeRF/evaluation.py takes PSNR / LPIPS / FID from pyiqa and has no call site this replaces; ops.ssim, mvip_nerf_amd/evaluate.py,
// the trainer's reference_ssim_lambda).
//
// Definition (conventions shared with tests/ssim_numpy.py).  x, y [N, H, W, C] fp32, channel-last, C in 1..4, H, W >= 11.
//   window: 11 taps g_k = e_k / sum_k e_k, e_k = exp(-(k-5)^2 / (2 1.5^2)), evaluated and summed (ascending) in fp64, rounded to
//   fp32; separable, "valid" extent: the map is [N, H-10, W-10, C], map pixel (i, j) is centred on image pixel (i+5, j+5).
//   per channel, F(v)(i, j) = sum_a g_a (sum_b g_b v(i+a, j+b)): along the row first, then down the column, taps ascending:
//     mx = F(x), my = F(y), exx = F(x x), eyy = F(y y), exy = F(x y)          (the products are formed first, in fp32)
//     mxx = mx mx, myy = my my, mxy = mx my;  sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy
//     n1 = 2 mxy + C1, n2 = 2 sxy + C2, d1 = (mxx + myy) + C1, d2 = (sxx + syy) + C2,  C1 = 1e-4, C2 = 9e-4 (data range 1)
//     s = (n1 n2) / (d1 d2)
//   No luminance conversion, no downsampling (this is not pyiqa's Y-channel preprocessing).
//   mask [N, H, W] bytes, optional: map pixel (i, j) counts iff mask(i+5, j+5) != 0 (without a mask every map pixel counts).
//   count_n = counted map pixels, ssim_n = (sum of s over counted pixels and channels) / (count_n C); count_n = 0: exactly 1.
// Gradient to x, for an upstream gradient gout [N]:
//     B = -s / d2,  Cp = (2 n1) / (d1 d2),  A = (((2 my) n2) / (d1 d2) - ((2 mx) s) / d1) - (2 mx) B - my Cp
//     gx(q) = scale_n ((G(A)(q) + (2 x_q) G(B)(q)) + y_q G(Cp)(q)),   scale_n = gout_n / (count_n C)   (count_n = 0: gx = 0)
//   G(P) is the "full" correlation with the same window: P zeroed where the map pixel is not counted and zero-padded by 10 on
//   every side, then F of that (image pixel q collects the map pixels q - (a, b), a, b in 0..10; the window is symmetric).
//
// Shape.  A tile is TX x TY = 32 x 16 pixels, a workgroup 256 threads (column = thread & 31, two rows each).
//   forward: one workgroup per map tile.  The (32+10) x (16+10) halo of x and y, all channels, is staged in LDS once
//     (coalesced along the row); per channel a horizontal pass writes five moment planes [26][32] to LDS and a vertical pass
//     leaves the thread's two map pixels in registers.  The map is written only when asked; A, B, Cp (zeroed off the mask) go to
//     the stash [3, N, H-10, W-10, C] only when the gradient is needed.  One fp64 partial sum and one count per workgroup: the
//     thread's values in ascending (channel, row) order, the six-step DPP tree per wave, the four wave totals in ascending order.
//   reduce: one workgroup per image; thread t adds the partials of its contiguous chunk in ascending order in fp64, thread 0 the
//     256 chunk totals in ascending order.  The partials of image n sit at [n T, (n+1) T): the layout depends on the image alone.
//   backward: one workgroup per image tile, a gather: the halo of the three stashed planes (zero outside the map) is staged,
//     the same two passes, a pointwise combine with x_q, y_q.  No atomics anywhere; no scratch.
// Every index is bounded before it is used (staging reads are guarded by the image / map extent, writes by the tile's valid
// part); offsets are 64-bit.  An image's result depends on its own inputs only: image n of a batch equals the single-image call
// bit for bit, and a call equals its repetition.
//
// Bytes per launch (E = N H W C, M = N (H-10)(W-10) C elements; halo re-reads are served by L2):
//   forward 8 E read (+ N H W mask bytes), 4 M written for the map, 12 M for the stash, 12 bytes per tile;
//   backward 12 M + 8 E read, 4 E written.  Recomputing the moments instead of the stash would save 24 M bytes and cost the
//   backward a 20-pixel halo of x and y and five more filter passes.
#include "common.h"

namespace mvip {
namespace ssim {

constexpr int BLOCK = 256;
constexpr int TX = 32, TY = 16;
constexpr int TAPS = 11, HALO = TAPS - 1;
constexpr int HX = TX + HALO, HY = TY + HALO;    // 42 x 26
constexpr int ROWS = TY / (BLOCK / TX);          // rows of the tile per thread: 2
constexpr float C1 = 1e-4f, C2 = 9e-4f;

// the window, fp64 -> fp32 (tests/ssim_numpy.py::window computes the same eleven values)
__device__ __forceinline__ constexpr float tap(int k) {
    constexpr float g[TAPS] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                               0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
    return g[k];
}

struct Shape {
    int H, W, MH, MW;                            // image and map extent
    int mtx, MT;                                 // map tiles per row of tiles, per image (forward)
    int itx, IT;                                 // image tiles (backward)
    long long HW, MHW;
};

// total over the workgroup, for thread 0 (the order is the file header's).  Every thread of the workgroup calls it.
__device__ __forceinline__ double block_sum(double v, double *lds) {
    const double w = dpp_wave_sum(v);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = w;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

template <int C>
__global__ __launch_bounds__(BLOCK) void forward_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                       const unsigned char *__restrict__ mask, const Shape s,
                                                       float *__restrict__ map, float *__restrict__ stash, const long long plane,
                                                       double *__restrict__ part, int *__restrict__ pcnt) {
    __shared__ float sx[HY][HX * C], sy[HY][HX * C];
    __shared__ float hm[5][HY][TX];
    __shared__ double red[BLOCK / MVIP_WAVE];
    __shared__ int cnt_lds;
    const int tid = threadIdx.x;
    const int n = blockIdx.x / s.MT, tile = blockIdx.x % s.MT;
    const int i0 = (tile / s.mtx) * TY, j0 = (tile % s.mtx) * TX;      // the tile's first map pixel = its halo's first image pixel
    if (tid == 0) cnt_lds = 0;
    // ---- the halo, all channels: rows i0 .. i0+25, columns j0 .. j0+41, zero outside the image
    const long long img = n * s.HW * C;
    const int rowlen = s.W * C;
    for (int idx = tid; idx < HY * HX * C; idx += BLOCK) {
        const int r = idx / (HX * C), cc = idx % (HX * C);
        const int iy = i0 + r, jc = j0 * C + cc;
        const bool in = iy < s.H && jc < rowlen;
        const long long off = img + (long long)iy * rowlen + jc;
        sx[r][cc] = in ? x[off] : 0.f;
        sy[r][cc] = in ? y[off] : 0.f;
    }
    __syncthreads();
    const int j = tid & (TX - 1), i = (tid / TX) * ROWS;
    const int mj = j0 + j;
    bool valid[ROWS], counted[ROWS];
    int cnt = 0;
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) {
        const int mi = i0 + i + rr;
        valid[rr] = mi < s.MH && mj < s.MW;
        counted[rr] = valid[rr] && (mask == nullptr || mask[n * s.HW + (long long)(mi + HALO / 2) * s.W + (mj + HALO / 2)] != 0);
        cnt += counted[rr];
    }
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        // ---- along the rows: five moment planes [26][32]
        for (int idx = tid; idx < HY * TX; idx += BLOCK) {
            const int r = idx / TX, jj = idx % TX;
            float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                const float xv = sx[r][(jj + k) * C + c], yv = sy[r][(jj + k) * C + c];
                a += tap(k) * xv;
                b += tap(k) * yv;
                aa += tap(k) * (xv * xv);
                bb += tap(k) * (yv * yv);
                ab += tap(k) * (xv * yv);
            }
            hm[0][r][jj] = a;
            hm[1][r][jj] = b;
            hm[2][r][jj] = aa;
            hm[3][r][jj] = bb;
            hm[4][r][jj] = ab;
        }
        __syncthreads();
        // ---- down the columns, into registers; the formula
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                mx += tap(k) * hm[0][i + rr + k][j];
                my += tap(k) * hm[1][i + rr + k][j];
                exx += tap(k) * hm[2][i + rr + k][j];
                eyy += tap(k) * hm[3][i + rr + k][j];
                exy += tap(k) * hm[4][i + rr + k][j];
            }
            if (!valid[rr]) continue;
            const float mxx = mx * mx, myy = my * my, mxy = mx * my;
            const float sxx = exx - mxx, syy = eyy - myy, sxy = exy - mxy;
            const float n1 = 2.f * mxy + C1, n2 = 2.f * sxy + C2, d1 = (mxx + myy) + C1, d2 = (sxx + syy) + C2;
            const float d12 = d1 * d2;
            const float sv = (n1 * n2) / d12;
            const long long p = ((n * s.MHW + (long long)(i0 + i + rr) * s.MW + mj)) * C + c;
            if (map != nullptr) map[p] = sv;
            if (stash != nullptr) {
                const float B = -sv / d2, Cp = (2.f * n1) / d12;
                const float A = ((((2.f * my) * n2) / d12 - ((2.f * mx) * sv) / d1) - (2.f * mx) * B) - my * Cp;
                stash[p] = counted[rr] ? A : 0.f;
                stash[plane + p] = counted[rr] ? B : 0.f;
                stash[2 * plane + p] = counted[rr] ? Cp : 0.f;
            }
            if (counted[rr]) acc += (double)sv;
        }
        __syncthreads();                         // hm is rewritten by the next channel
    }
    if (cnt) atomicAdd(&cnt_lds, cnt);           // an integer count in LDS: exact in any order
    const double total = block_sum(acc, red);    // its barrier also orders the count
    if (tid == 0) {
        part[blockIdx.x] = total;
        pcnt[blockIdx.x] = cnt_lds;
    }
}

// one workgroup per image: the image's partials in ascending order, in fp64
__global__ __launch_bounds__(BLOCK) void reduce_kernel(const double *__restrict__ part, const int *__restrict__ pcnt, const int T,
                                                      const int C, float *__restrict__ ssim, int *__restrict__ count) {
    __shared__ double s_sum[BLOCK];
    __shared__ int s_cnt[BLOCK];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int chunk = (T + BLOCK - 1) / BLOCK, lo = min(tid * chunk, T), hi = min(lo + chunk, T);
    const double *pp = part + (long long)n * T;
    const int *pc = pcnt + (long long)n * T;
    double a = 0.0;
    int c = 0;
    for (int t = lo; t < hi; ++t) { a += pp[t]; c += pc[t]; }
    s_sum[tid] = a;
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        int cnt = 0;
        for (int t = 0; t < BLOCK; ++t) { total += s_sum[t]; cnt += s_cnt[t]; }
        ssim[n] = cnt > 0 ? (float)(total / ((double)cnt * (double)C)) : 1.0f;
        count[n] = cnt;
    }
}

template <int C>
__global__ __launch_bounds__(BLOCK) void backward_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                        const float *__restrict__ stash, const long long plane,
                                                        const float *__restrict__ gout, const int *__restrict__ count, const Shape s,
                                                        float *__restrict__ gx) {
    __shared__ float sp[3][HY][HX * C];
    __shared__ float hm[3][HY][TX];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / s.IT, tile = blockIdx.x % s.IT;
    const int q0y = (tile / s.itx) * TY, q0x = (tile % s.itx) * TX;
    const int j = tid & (TX - 1), i = (tid / TX) * ROWS;
    const int qx = q0x + j;
    const long long img = n * s.HW * C;
    const int cnt = count[n];
    if (cnt == 0) {                              // uniform over the workgroup: an empty mask gives an all-zero gradient
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const int qy = q0y + i + rr;
            if (qy < s.H && qx < s.W)
                for (int c = 0; c < C; ++c) gx[img + ((long long)qy * s.W + qx) * C + c] = 0.f;
        }
        return;
    }
    const float scale = gout[n] / (float)(cnt * C);
    // ---- the halo of the three planes: map rows q0y-10 .. q0y+15, columns q0x-10 .. q0x+31, zero outside the map
    const long long mp = n * s.MHW * C;
    const int rowlen = s.MW * C;
    for (int idx = tid; idx < HY * HX * C; idx += BLOCK) {
        const int r = idx / (HX * C), cc = idx % (HX * C);
        const int mi = q0y - HALO + r, mjc = (q0x - HALO) * C + cc;
        const bool in = mi >= 0 && mi < s.MH && mjc >= 0 && mjc < rowlen;
        const long long off = mp + (long long)mi * rowlen + mjc;
        sp[0][r][cc] = in ? stash[off] : 0.f;
        sp[1][r][cc] = in ? stash[plane + off] : 0.f;
        sp[2][r][cc] = in ? stash[2 * plane + off] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        for (int idx = tid; idx < HY * TX; idx += BLOCK) {
            const int r = idx / TX, jj = idx % TX;
            float a = 0.f, b = 0.f, cp = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                a += tap(k) * sp[0][r][(jj + k) * C + c];
                b += tap(k) * sp[1][r][(jj + k) * C + c];
                cp += tap(k) * sp[2][r][(jj + k) * C + c];
            }
            hm[0][r][jj] = a;
            hm[1][r][jj] = b;
            hm[2][r][jj] = cp;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            float ga = 0.f, gb = 0.f, gc = 0.f;
#pragma unroll
            for (int k = 0; k < TAPS; ++k) {
                ga += tap(k) * hm[0][i + rr + k][j];
                gb += tap(k) * hm[1][i + rr + k][j];
                gc += tap(k) * hm[2][i + rr + k][j];
            }
            const int qy = q0y + i + rr;
            if (qy < s.H && qx < s.W) {
                const long long q = img + ((long long)qy * s.W + qx) * C + c;
                gx[q] = scale * ((ga + (2.f * x[q]) * gb) + y[q] * gc);
            }
        }
        __syncthreads();
    }
}

}  // namespace ssim
}  // namespace mvip

using namespace mvip;

constexpr int SSIM_MAX_SIDE = 16384;

// false: bad shape.  N * (tiles per image) -- the grids and the partial arrays -- must fit an int.
static inline bool ssim_shape(int64_t N, int H, int W, int C, ssim::Shape &s) {
    if (N < 0 || H < ssim::TAPS || W < ssim::TAPS || H > SSIM_MAX_SIDE || W > SSIM_MAX_SIDE || C < 1 || C > 4) return false;
    s.H = H;
    s.W = W;
    s.MH = H - ssim::HALO;
    s.MW = W - ssim::HALO;
    s.mtx = (s.MW + ssim::TX - 1) / ssim::TX;
    s.MT = s.mtx * ((s.MH + ssim::TY - 1) / ssim::TY);
    s.itx = (W + ssim::TX - 1) / ssim::TX;
    s.IT = s.itx * ((H + ssim::TY - 1) / ssim::TY);
    s.HW = (long long)H * W;
    s.MHW = (long long)s.MH * s.MW;
    return N <= (int64_t)INT32_MAX / s.IT;       // IT >= MT
}

extern "C" int64_t mvip_ssim_tiles(int H, int W) {
    ssim::Shape s;
    return ssim_shape(0, H, W, 1, s) ? s.MT : -1;
}

extern "C" int mvip_ssim_forward(const float *x, const float *y, const void *mask, int64_t N, int H, int W, int C, float *map,
                                 float *stash, double *partials, int *partial_counts, float *ssim_out, int *count, void *stream) {
    ssim::Shape s;
    if (!ssim_shape(N, H, W, C, s)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!x || !y || !partials || !partial_counts || !ssim_out || !count) return MVIP_EINVAL;
    const long long plane = N * s.MHW * C;
    const dim3 grid((unsigned)(N * s.MT)), block(ssim::BLOCK);
    const unsigned char *m = (const unsigned char *)mask;
#define MVIP_SSIM_FWD(CH)                                                                                                       \
    hipLaunchKernelGGL(ssim::forward_kernel<CH>, grid, block, 0, as_stream(stream), x, y, m, s, map, stash, plane, partials,    \
                       partial_counts)
    switch (C) {
        case 1: MVIP_SSIM_FWD(1); break;
        case 2: MVIP_SSIM_FWD(2); break;
        case 3: MVIP_SSIM_FWD(3); break;
        default: MVIP_SSIM_FWD(4); break;
    }
#undef MVIP_SSIM_FWD
    hipLaunchKernelGGL(ssim::reduce_kernel, dim3((unsigned)N), block, 0, as_stream(stream), (const double *)partials,
                       (const int *)partial_counts, s.MT, C, ssim_out, count);
    return check_launch();
}

extern "C" int mvip_ssim_backward(const float *x, const float *y, const float *stash, const float *gout, const int *count,
                                  int64_t N, int H, int W, int C, float *gx, void *stream) {
    ssim::Shape s;
    if (!ssim_shape(N, H, W, C, s)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!x || !y || !stash || !gout || !count || !gx || gx == x || gx == y) return MVIP_EINVAL;
    const long long plane = N * s.MHW * C;
    const dim3 grid((unsigned)(N * s.IT)), block(ssim::BLOCK);
#define MVIP_SSIM_BWD(CH) \
    hipLaunchKernelGGL(ssim::backward_kernel<CH>, grid, block, 0, as_stream(stream), x, y, stash, plane, gout, count, s, gx)
    switch (C) {
        case 1: MVIP_SSIM_BWD(1); break;
        case 2: MVIP_SSIM_BWD(2); break;
        case 3: MVIP_SSIM_BWD(3); break;
        default: MVIP_SSIM_BWD(4); break;
    }
#undef MVIP_SSIM_BWD
    return check_launch();
}
