// Harmonic hole filling of rendered disparity maps, and 2D mask dilation (beyond the reference, which takes its
// Depth_inpainted/ targets as given; stands in for --prepare + LaMa; ops.harmonic_fill, ops.mask_dilate2d, mvip_nerf_amd/prepare.py).
//
// Definition, per image v [H, W] fp32 with mask m [H, W] (conventions shared with tests/harmonic_numpy.py):
//   U = m or {p : v_p not finite} (the unknowns), K the rest;  N(p) = the 4-neighbours of p inside the image, deg(p) = |N(p)|;
//   for p in U:  deg(p) u_p - sum_{q in N(p) and U} u_q = b_p,   b_p = sum_{q in N(p) and K} v_q  (added in the order up, left,
//   right, down in fp32);  output = v bit for bit on K, u on U.  U empty: nothing to do.  U = the whole image: singular, the
//   image is returned as it is.  Images of a batch are independent problems.
//
// The guided (Poisson) variant (ops.poisson_fill, prepare.propagate_reference(blend='poisson'); conventions shared with
// tests/poisson_numpy.py) adds a guide g [H, W] fp32 and labels l [H, W] int32 per image; U, K, N(p), deg(p) as above.  An edge
// (p, q), q in N(p), is GUIDED iff l_p >= 0, l_q == l_p, and g_p, g_q are both finite.  For p in U:
//   deg(p) u_p - sum_{q in N(p) and U} u_q = b_p,   b_p = s_p + t_p,
//   s_p = sum_{q in N(p) and K} v_q                  (the right-hand side above, the same order and precision),
//   t_p = sum_{q in N(p), (p, q) guided} (g_p - g_q)  (an fp32 subtraction, then an fp32 addition, up, left, right, down, from 0.f);
//   output = v bit for bit on K, u on U; U empty / everything as above.  The guide's gradients are trusted inside one source
//   (one label) only: across a change of label, and where there is none (-1), the edge keeps the harmonic zero-gradient
//   condition.  With no guided edge t_p = 0.f and b_p is the harmonic fill's bit for bit (s_p is never -0).  Only the
//   right-hand side differs: poisson_init_kernel stands in for init_kernel, everything else is shared.
//
// Method: conjugate gradients with the Jacobi preconditioner (z = r / deg) from u = 0, stopped per image when
// r.z <= eps^2 r0.z0 on the recursively updated residual.
//
// Shape: the image is cut into TILES of 64 x 16 pixels (lane = column, each of the four waves four rows); only the tiles that
// hold an unknown ("active") are ever visited again after the set-up, through a per-image list in raster order.  All vectors
// (r, z, two copies of p, Ap) are image-shaped arrays in the caller's workspace that are touched at unknown pixels only;
// u lives in the output image.  Every cross-workgroup dependency is a launch boundary: no grid barrier, no spin, no
// cooperative launch.  One iteration k is two launches over (image, active tile):
//   stencil:  rz = sum of the image's r.z partials;  frozen for good if !(rz > eps^2 rz0)  (the partials are not written again,
//             so every later launch decides the same);  beta = rz / rz_prev (0 in iteration 0);  p' = z + beta p is formed
//             for the tile's pixels AND their neighbours from z and the previous copy of p (the same expression in the same
//             precision on both sides of a tile edge, so what a neighbour computes is what the owner stores), written to
//             the other copy of p;  Ap = deg p' - sum of the unknown neighbours' p';  partial of p'.Ap.
//   update:   alpha = rz / (sum of the image's p.Ap partials);  u += alpha p;  r -= alpha Ap;  z = r / deg;  partial of r.z.
// The scalars live on the device in state[n] (16 words per image): the tile with list index 0 writes rz, rz0, the iteration count
// and the done flag; they are only read by LATER launches.  A frozen image divides nothing.
//
// Summation order, fixed: a tile's partial is lane sums (rows in ascending order) -> six-step DPP tree per wave -> the four
// wave totals added in ascending order.  An image's total is re-reduced by every consumer workgroup in the same way: thread t
// adds the partials t, t + 256, ... in ascending order, then the same tree.  The partials of image n sit at
// [n * T + j], j the index in that image's active list: the layout depends on the image alone, so image n of a batch is
// bit-equal to the single-image call, and two calls are bit-equal.  No float atomics; the only atomics are integer counts in
// LDS during the set-up.  No scratch.
//
// Bytes per unknown-tile pixel and iteration: stencil 1 (mask) + 8 read (z, p; the neighbours' come from cache) + 8 written,
// update 1 + 16 read (u, r, p, Ap) + 12 written.
#include "common.h"

namespace mvip {
namespace harmonic {

constexpr int BLOCK = 256;
constexpr int TX = 64, TY = 16;                  // tile: 64 columns (the lanes) x 16 rows (4 per wave)
constexpr int ROWS = TY / (BLOCK / MVIP_WAVE);
constexpr int STATE = 16;                        // 32-bit words of state per image
enum { S_NACT = 0, S_UNKNOWNS, S_SINGULAR, S_DONE, S_ITERS, S_RZ0, S_RZA, S_RZB, S_RESIDUAL, S_CONVERGED };

struct Shape {
    int H, W, tx, T;                             // tx tiles per row of tiles, T tiles per image
    long long HW;
};

struct Work {                                    // the caller's workspace, carved in this order
    float *part_rz, *part_pap;                   // [N * T]
    int *tile_count, *act;                       // [N * T]
    float *r, *z, *p0, *p1, *ap;                 // [N * H * W]
    unsigned char *um;                           // [N * H * W]
};

__device__ __forceinline__ float as_f(int v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ int as_i(float v) { return __builtin_bit_cast(int, v); }

// total over the workgroup in every thread; the order is the file header's.  Every thread of the workgroup calls it.
__device__ __forceinline__ float block_sum(float v, float *lds) {
    const float w = dpp_wave_sum(v);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = w;
    __syncthreads();
    const float t = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    __syncthreads();
    return t;
}
__device__ __forceinline__ float block_max(float v, float *lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
    __syncthreads();
    return t;
}
__device__ __forceinline__ float image_sum(const float *part, int n, float *lds) {
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += BLOCK) a += part[i];
    return block_sum(a, lds);
}
__device__ __forceinline__ int degree(const Shape &s, int x, int y) {
    return (y > 0) + (y < s.H - 1) + (x > 0) + (x < s.W - 1);
}

// ---- set-up ------------------------------------------------------------------------------------------------------------
// every tile of every image: mark U, copy the image to the output, count the tile's unknowns
__global__ __launch_bounds__(BLOCK) void mark_kernel(const float *__restrict__ v, const unsigned char *__restrict__ m, const Shape s,
                                                    float *__restrict__ out, const Work w) {
    __shared__ int cnt;
    const int n = blockIdx.x / s.T, t = blockIdx.x % s.T;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int x = (t % s.tx) * TX + lane_id(), y0 = (t / s.tx) * TY + (threadIdx.x >> 6) * ROWS;
    int c = 0;
    if (x < s.W) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = y0 + i;
            if (y >= s.H) break;
            const long long p = n * s.HW + (long long)y * s.W + x;
            const float val = v[p];
            const bool u = m[p] != 0 || !finite(val);
            w.um[p] = u ? 1 : 0;
            out[p] = val;
            c += u;
        }
    }
    if (c) atomicAdd(&cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) w.tile_count[blockIdx.x] = cnt;
}

// one workgroup per image: the active tiles in raster order, the unknown count, the state
__global__ __launch_bounds__(BLOCK) void list_kernel(const Shape s, const Work w, int *__restrict__ state) {
    __shared__ int s_act[BLOCK], s_unk[BLOCK];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int chunk = (s.T + BLOCK - 1) / BLOCK, lo = min(tid * chunk, s.T), hi = min(lo + chunk, s.T);
    const int *tc = w.tile_count + (long long)n * s.T;
    int a = 0, u = 0;
    for (int t = lo; t < hi; ++t) { a += tc[t] > 0; u += tc[t]; }
    s_act[tid] = a;
    s_unk[tid] = u;
    __syncthreads();
    int off = 0, nact = 0, unknowns = 0;
    for (int i = 0; i < BLOCK; ++i) {            // 256 LDS words, the same walk in every thread
        if (i == tid) off = nact;
        nact += s_act[i];
        unknowns += s_unk[i];
    }
    int *al = w.act + (long long)n * s.T;
    for (int t = lo; t < hi; ++t)
        if (tc[t] > 0) al[off++] = t;
    if (tid == 0) {
        const bool singular = unknowns == s.HW;
        int *st = state + n * STATE;
        st[S_NACT] = singular ? 0 : nact;
        st[S_UNKNOWNS] = unknowns;
        st[S_SINGULAR] = singular;
        st[S_DONE] = singular || nact == 0;
        st[S_ITERS] = 0;
        st[S_RZ0] = st[S_RZA] = st[S_RZB] = as_i(0.f);
        st[S_RESIDUAL] = as_i(0.f);
        st[S_CONVERGED] = 0;
#pragma unroll
        for (int i = S_CONVERGED + 1; i < STATE; ++i) st[i] = 0;
    }
}

// (image, list index) of a workgroup of the per-active-tile launches, and the tile's pixel column / first row of the thread
struct Where {
    int n, j, x, y0;
    bool live;
};
__device__ __forceinline__ Where where(const Shape &s, const Work &w, const int *state, int max_act) {
    Where q;
    q.n = blockIdx.x / max_act;
    q.j = blockIdx.x % max_act;
    q.live = q.j < state[q.n * STATE + S_NACT];
    const int t = q.live ? w.act[(long long)q.n * s.T + q.j] : 0;
    q.x = (t % s.tx) * TX + lane_id();
    q.y0 = (t / s.tx) * TY + (threadIdx.x >> 6) * ROWS;
    return q;
}

// u = 0, r = b, z = b / deg on the unknowns of the active tiles; partial of r.z
__global__ __launch_bounds__(BLOCK) void init_kernel(const float *__restrict__ v, const Shape s, float *__restrict__ out, const Work w,
                                                    const int *__restrict__ state, int max_act) {
    __shared__ float lds[BLOCK / MVIP_WAVE];
    const Where q = where(s, w, state, max_act);
    if (!q.live) return;                         // uniform over the workgroup
    const long long base = q.n * s.HW;
    float acc = 0.f;
    if (q.x < s.W) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = q.y0 + i;
            if (y >= s.H) break;
            const long long p = base + (long long)y * s.W + q.x;
            if (!w.um[p]) continue;
            float b = 0.f;
            if (y > 0 && !w.um[p - s.W]) b += v[p - s.W];
            if (q.x > 0 && !w.um[p - 1]) b += v[p - 1];
            if (q.x < s.W - 1 && !w.um[p + 1]) b += v[p + 1];
            if (y < s.H - 1 && !w.um[p + s.W]) b += v[p + s.W];
            const float z = b / (float)degree(s, q.x, y);
            out[p] = 0.f;
            w.r[p] = b;
            w.z[p] = z;
            acc += b * z;
        }
    }
    const float total = block_sum(acc, lds);
    if (threadIdx.x == 0) w.part_rz[(long long)q.n * s.T + q.j] = total;
}

// the guided right-hand side (the file header's Poisson variant): init_kernel with b = s + t, t the sum of g_p - g_q over the
// guided edges.  g and l are read at the pixel and its four neighbours only, every index inside the image.
__global__ __launch_bounds__(BLOCK) void poisson_init_kernel(const float *__restrict__ v, const float *__restrict__ g,
                                                            const int *__restrict__ l, const Shape s, float *__restrict__ out, const Work w,
                                                            const int *__restrict__ state, int max_act) {
    __shared__ float lds[BLOCK / MVIP_WAVE];
    const Where q = where(s, w, state, max_act);
    if (!q.live) return;                         // uniform over the workgroup
    const long long base = q.n * s.HW;
    float acc = 0.f;
    if (q.x < s.W) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = q.y0 + i;
            if (y >= s.H) break;
            const long long p = base + (long long)y * s.W + q.x;
            if (!w.um[p]) continue;
            float b = 0.f;
            if (y > 0 && !w.um[p - s.W]) b += v[p - s.W];
            if (q.x > 0 && !w.um[p - 1]) b += v[p - 1];
            if (q.x < s.W - 1 && !w.um[p + 1]) b += v[p + 1];
            if (y < s.H - 1 && !w.um[p + s.W]) b += v[p + s.W];
            const float gp = g[p];
            const int lp = l[p];
            float t = 0.f;
            if (lp >= 0 && finite(gp)) {
                // the edge (p, o) is guided iff o carries p's label and a finite guide
                auto edge = [&](long long o) -> void {
                    const float gq = g[o];
                    if (l[o] == lp && finite(gq)) t += gp - gq;
                };
                if (y > 0) edge(p - s.W);
                if (q.x > 0) edge(p - 1);
                if (q.x < s.W - 1) edge(p + 1);
                if (y < s.H - 1) edge(p + s.W);
            }
            b += t;                              // t == 0.f leaves the harmonic b bit for bit (b is never -0)
            const float z = b / (float)degree(s, q.x, y);
            out[p] = 0.f;
            w.r[p] = b;
            w.z[p] = z;
            acc += b * z;
        }
    }
    const float total = block_sum(acc, lds);
    if (threadIdx.x == 0) w.part_rz[(long long)q.n * s.T + q.j] = total;
}

// ---- one CG iteration: two launches ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void stencil_kernel(const Shape s, const Work w, int *state, int max_act, int first, int parity,
                                                       float eps2) {
    __shared__ float lds[BLOCK / MVIP_WAVE];
    const Where q = where(s, w, state, max_act);
    if (!q.live) return;
    int *st = state + q.n * STATE;
    const int nact = st[S_NACT];
    const float rz = image_sum(w.part_rz + (long long)q.n * s.T, nact, lds);
    const float rz0 = first ? rz : as_f(st[S_RZ0]);
    if (!(rz > eps2 * rz0)) {                    // converged (or not a number): frozen from here on, the same verdict in every launch
        if (q.j == 0 && threadIdx.x == 0) st[S_DONE] = 1;
        return;
    }
    const float beta = first ? 0.f : rz / as_f(st[parity ? S_RZA : S_RZB]);      // the previous iteration's r.z
    if (q.j == 0 && threadIdx.x == 0) {          // read by later launches only
        st[parity ? S_RZB : S_RZA] = as_i(rz);
        if (first) st[S_RZ0] = as_i(rz);
        st[S_ITERS] += 1;
    }
    const float *pc = parity ? w.p1 : w.p0;      // the previous copy (iteration k - 1 wrote it), unread in iteration 0
    float *pn = parity ? w.p0 : w.p1;
    const long long base = q.n * s.HW;
    // p' of a pixel: 0 off the unknowns
    auto pnew = [&](long long p) -> float {
        if (!w.um[p]) return 0.f;
        const float z = w.z[p];
        return first ? z : z + beta * pc[p];
    };
    float acc = 0.f;
    if (q.x < s.W) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = q.y0 + i;
            if (y >= s.H) break;
            const long long p = base + (long long)y * s.W + q.x;
            if (!w.um[p]) continue;
            const float c = pnew(p);
            float nb = 0.f;
            if (y > 0) nb += pnew(p - s.W);
            if (q.x > 0) nb += pnew(p - 1);
            if (q.x < s.W - 1) nb += pnew(p + 1);
            if (y < s.H - 1) nb += pnew(p + s.W);
            const float ap = (float)degree(s, q.x, y) * c - nb;
            pn[p] = c;
            w.ap[p] = ap;
            acc += c * ap;
        }
    }
    const float total = block_sum(acc, lds);
    if (threadIdx.x == 0) w.part_pap[(long long)q.n * s.T + q.j] = total;
}

__global__ __launch_bounds__(BLOCK) void update_kernel(const Shape s, float *__restrict__ out, const Work w, const int *__restrict__ state,
                                                      int max_act, int parity) {
    __shared__ float lds[BLOCK / MVIP_WAVE];
    const Where q = where(s, w, state, max_act);
    if (!q.live) return;
    const int *st = state + q.n * STATE;
    if (st[S_DONE]) return;                      // set by an earlier launch; uniform over the image
    const float pap = image_sum(w.part_pap + (long long)q.n * s.T, st[S_NACT], lds);
    const float alpha = as_f(st[parity ? S_RZB : S_RZA]) / pap;
    const float *pn = parity ? w.p0 : w.p1;
    const long long base = q.n * s.HW;
    float acc = 0.f;
    if (q.x < s.W) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = q.y0 + i;
            if (y >= s.H) break;
            const long long p = base + (long long)y * s.W + q.x;
            if (!w.um[p]) continue;
            const float r = w.r[p] - alpha * w.ap[p];
            const float z = r / (float)degree(s, q.x, y);
            out[p] += alpha * pn[p];
            w.r[p] = r;
            w.z[p] = z;
            acc += r * z;
        }
    }
    const float total = block_sum(acc, lds);
    if (threadIdx.x == 0) w.part_rz[(long long)q.n * s.T + q.j] = total;
}

// ---- the end: true residual (max-norm, for the record), the verdict ----------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void residual_kernel(const Shape s, const float *__restrict__ out, const Work w,
                                                        const int *__restrict__ state, int max_act) {
    __shared__ float lds[BLOCK / MVIP_WAVE];
    const Where q = where(s, w, state, max_act);
    if (!q.live) return;
    const long long base = q.n * s.HW;
    float worst = 0.f;
    if (q.x < s.W) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int y = q.y0 + i;
            if (y >= s.H) break;
            const long long p = base + (long long)y * s.W + q.x;
            if (!w.um[p]) continue;
            float nb = 0.f;
            if (y > 0) nb += out[p - s.W];
            if (q.x > 0) nb += out[p - 1];
            if (q.x < s.W - 1) nb += out[p + 1];
            if (y < s.H - 1) nb += out[p + s.W];
            const float d = (float)degree(s, q.x, y);
            const float e = fabsf(nb - d * out[p]) / d;
            worst = e > worst || e != e ? e : worst;         // a NaN is reported, not dropped
        }
    }
    const bool nan = __syncthreads_or(worst != worst);
    const float total = block_max(worst == worst ? worst : 0.f, lds);
    if (threadIdx.x == 0) w.part_pap[(long long)q.n * s.T + q.j] = nan ? __builtin_nanf("") : total;
}

__global__ __launch_bounds__(BLOCK) void verdict_kernel(const Shape s, const Work w, int *state, float eps2) {
    __shared__ float lds[BLOCK / MVIP_WAVE];
    int *st = state + blockIdx.x * STATE;
    const int nact = st[S_NACT];
    const float rz = image_sum(w.part_rz + (long long)blockIdx.x * s.T, nact, lds);
    const float *pm = w.part_pap + (long long)blockIdx.x * s.T;
    float worst = 0.f;
    bool nan = false;
    for (int i = threadIdx.x; i < nact; i += BLOCK) {
        const float e = pm[i];
        nan |= e != e;
        worst = fmaxf(worst, e);
    }
    nan = __syncthreads_or(nan);
    worst = block_max(worst, lds);
    if (threadIdx.x == 0) {
        st[S_RESIDUAL] = as_i(nan ? __builtin_nanf("") : worst);
        st[S_CONVERGED] = !st[S_SINGULAR] && (nact == 0 || (st[S_ITERS] > 0 ? rz <= eps2 * as_f(st[S_RZ0]) : rz == 0.f));
    }
}

// ---- 2D dilation: one round --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void dilate2d_kernel(const unsigned char *__restrict__ in, long long total, int H, int W,
                                                        unsigned char *__restrict__ out) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= total) return;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    unsigned char v = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        if (y + dy < 0 || y + dy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            if (x + dx < 0 || x + dx >= W) continue;
            v |= in[p + (long long)dy * W + dx];
        }
    }
    out[p] = v ? 1 : 0;
}

}  // namespace harmonic
}  // namespace mvip

using namespace mvip;

constexpr int HARMONIC_MAX_SIDE = 16384;

// false: bad shape.  N * T (the workgroups of the set-up, the partial arrays) must fit an int.
static inline bool harmonic_shape(int64_t N, int H, int W, harmonic::Shape &s) {
    if (N < 0 || H < 1 || W < 1 || H > HARMONIC_MAX_SIDE || W > HARMONIC_MAX_SIDE) return false;
    s.H = H;
    s.W = W;
    s.tx = (W + harmonic::TX - 1) / harmonic::TX;
    s.T = s.tx * ((H + harmonic::TY - 1) / harmonic::TY);
    s.HW = (long long)H * W;
    return N <= (int64_t)INT32_MAX / s.T && N <= (int64_t)INT32_MAX / harmonic::STATE;
}
static inline int64_t harmonic_align(int64_t b) { return (b + 255) / 256 * 256; }
static inline harmonic::Work harmonic_carve(void *workspace, int64_t N, const harmonic::Shape &s) {
    char *c = (char *)workspace;
    const int64_t tiles = harmonic_align(N * s.T * 4), px = harmonic_align(N * s.HW * 4);
    harmonic::Work w;
    w.part_rz = (float *)c;            c += tiles;
    w.part_pap = (float *)c;           c += tiles;
    w.tile_count = (int *)c;           c += tiles;
    w.act = (int *)c;                  c += tiles;
    w.r = (float *)c;                  c += px;
    w.z = (float *)c;                  c += px;
    w.p0 = (float *)c;                 c += px;
    w.p1 = (float *)c;                 c += px;
    w.ap = (float *)c;                 c += px;
    w.um = (unsigned char *)c;
    return w;
}
static inline bool harmonic_grid(int64_t N, int64_t max_act, const harmonic::Shape &s) {
    return max_act >= 0 && max_act <= s.T && (max_act == 0 || N <= (int64_t)INT32_MAX / max_act);
}

extern "C" int64_t mvip_harmonic_tiles(int H, int W) {
    harmonic::Shape s;
    return harmonic_shape(0, H, W, s) ? s.T : -1;
}

extern "C" int64_t mvip_harmonic_workspace_bytes(int64_t N, int H, int W) {
    harmonic::Shape s;
    if (!harmonic_shape(N, H, W, s)) return -1;
    return 4 * harmonic_align(N * s.T * 4) + 5 * harmonic_align(N * s.HW * 4) + harmonic_align(N * s.HW);
}

extern "C" int mvip_harmonic_setup(const float *values, const void *masks, int64_t N, int H, int W, float *out, void *workspace,
                                   int *state, void *stream) {
    harmonic::Shape s;
    if (!harmonic_shape(N, H, W, s)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!values || !masks || !out || !workspace || !state || out == values) return MVIP_EINVAL;
    const harmonic::Work w = harmonic_carve(workspace, N, s);
    hipLaunchKernelGGL(harmonic::mark_kernel, dim3((unsigned)(N * s.T)), dim3(harmonic::BLOCK), 0, as_stream(stream), values,
                       (const unsigned char *)masks, s, out, w);
    hipLaunchKernelGGL(harmonic::list_kernel, dim3((unsigned)N), dim3(harmonic::BLOCK), 0, as_stream(stream), s, w, state);
    return check_launch();
}

extern "C" int mvip_harmonic_init(const float *values, int64_t N, int H, int W, float *out, void *workspace, const int *state,
                                  int64_t max_act, void *stream) {
    harmonic::Shape s;
    if (!harmonic_shape(N, H, W, s) || !harmonic_grid(N, max_act, s)) return MVIP_EINVAL;
    if (N == 0 || max_act == 0) return MVIP_OK;
    if (!values || !out || !workspace || !state || out == values) return MVIP_EINVAL;
    hipLaunchKernelGGL(harmonic::init_kernel, dim3((unsigned)(N * max_act)), dim3(harmonic::BLOCK), 0, as_stream(stream), values, s,
                       out, harmonic_carve(workspace, N, s), state, (int)max_act);
    return check_launch();
}

extern "C" int mvip_poisson_init(const float *values, const float *guide, const int *labels, int64_t N, int H, int W, float *out,
                                 void *workspace, const int *state, int64_t max_act, void *stream) {
    harmonic::Shape s;
    if (!harmonic_shape(N, H, W, s) || !harmonic_grid(N, max_act, s)) return MVIP_EINVAL;
    if (N == 0 || max_act == 0) return MVIP_OK;
    if (!values || !guide || !labels || !out || !workspace || !state || out == values) return MVIP_EINVAL;
    hipLaunchKernelGGL(harmonic::poisson_init_kernel, dim3((unsigned)(N * max_act)), dim3(harmonic::BLOCK), 0, as_stream(stream),
                       values, guide, labels, s, out, harmonic_carve(workspace, N, s), state, (int)max_act);
    return check_launch();
}

extern "C" int mvip_harmonic_iterate(int64_t N, int H, int W, float *out, void *workspace, int *state, int64_t max_act,
                                     int first_iteration, int iterations, float eps, void *stream) {
    harmonic::Shape s;
    if (!harmonic_shape(N, H, W, s) || !harmonic_grid(N, max_act, s) || first_iteration < 0 || iterations < 0 ||
        first_iteration > INT32_MAX - iterations || !(eps >= 0.f) || !(eps < 1.f))
        return MVIP_EINVAL;
    if (N == 0 || max_act == 0 || iterations == 0) return MVIP_OK;
    if (!out || !workspace || !state) return MVIP_EINVAL;
    const harmonic::Work w = harmonic_carve(workspace, N, s);
    const dim3 grid((unsigned)(N * max_act)), block(harmonic::BLOCK);
    for (int k = first_iteration; k < first_iteration + iterations; ++k) {
        hipLaunchKernelGGL(harmonic::stencil_kernel, grid, block, 0, as_stream(stream), s, w, state, (int)max_act, k == 0 ? 1 : 0,
                           k & 1, eps * eps);
        hipLaunchKernelGGL(harmonic::update_kernel, grid, block, 0, as_stream(stream), s, out, w, (const int *)state, (int)max_act,
                           k & 1);
    }
    return check_launch();
}

extern "C" int mvip_harmonic_finish(int64_t N, int H, int W, const float *out, void *workspace, int *state, int64_t max_act,
                                    float eps, void *stream) {
    harmonic::Shape s;
    if (!harmonic_shape(N, H, W, s) || !harmonic_grid(N, max_act, s) || !(eps >= 0.f) || !(eps < 1.f)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!out || !workspace || !state) return MVIP_EINVAL;
    const harmonic::Work w = harmonic_carve(workspace, N, s);
    if (max_act > 0)
        hipLaunchKernelGGL(harmonic::residual_kernel, dim3((unsigned)(N * max_act)), dim3(harmonic::BLOCK), 0, as_stream(stream), s,
                           out, w, (const int *)state, (int)max_act);
    hipLaunchKernelGGL(harmonic::verdict_kernel, dim3((unsigned)N), dim3(harmonic::BLOCK), 0, as_stream(stream), s, w, state,
                       eps * eps);
    return check_launch();
}

extern "C" int mvip_mask_dilate2d(const void *masks_in, int64_t N, int H, int W, void *masks_out, void *stream) {
    harmonic::Shape s;
    if (!harmonic_shape(N, H, W, s) || N * s.HW > (int64_t)INT32_MAX * harmonic::BLOCK) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!masks_in || !masks_out || masks_in == masks_out) return MVIP_EINVAL;
    const long long total = N * s.HW;
    hipLaunchKernelGGL(harmonic::dilate2d_kernel, dim3((unsigned)((total + harmonic::BLOCK - 1) / harmonic::BLOCK)),
                       dim3(harmonic::BLOCK), 0, as_stream(stream), (const unsigned char *)masks_in, total, H, W,
                       (unsigned char *)masks_out);
    return check_launch();
}
