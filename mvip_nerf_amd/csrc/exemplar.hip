// Exemplar-based (PatchMatch) image inpainting (beyond the reference, whose RGB_inpainted/ images are made elsewhere by LaMa;
// ops.exemplar_fill, prepare.inpaint_views, propagate_reference(fill='exemplar')).  A weight-free, textured 2D fill: a pyramid,
// then nearest-neighbour-field (NNF) search alternating with voting, coarse to fine.  After the quantisation everything is
// integer arithmetic; the definition is stated once more, vectorised in numpy, in tests/exemplar_numpy.py, and the two agree
// bit for bit.
//
// Definition, per image [H, W, 3] fp32 with mask [H, W] (and optionally sources [H, W]), patch side P odd in 3..9, r = P / 2:
//   quantise  q = rint(clip(v, 0, 1) * 255) in fp32; a pixel with a non-finite channel joins the hole; hole pixels start as 0.
//             bad = hole, or outside `sources`.  One RGBX word per pixel (X = 0).
//   sets      a centre is inside if its patch lies in the image;  T = inside centres whose patch holds a hole pixel;  S = inside
//             centres whose patch holds no bad pixel (a separable box test: a row pass, then a column pass).  S empty at level 0:
//             singular, the image is returned as it is.
//   pyramid   level l + 1 is [h / 2, w / 2] (an odd last row / column is dropped): colour = (2 sum + n) / (2 n) over the n KNOWN
//             pixels of the 2 x 2 block (0 for n = 0), hole = any of the four is hole, bad = any of the four is bad.  The batch
//             shares the geometric level count (levels are added while min(h, w) / 2 >= 4 P, up to max_levels); an image uses the
//             leading levels that still have a source and starts at the coarsest of them.
//   hash      lowbias32 chained over (seed ^ 0x9e3779b9, level, iteration, k, pixel = y w + x at that level), uint32.
//   initial   coarsest level: s(t) = the (hash mod |S|)-th source in raster order (iteration = 0xffffffff, k = 0).  Finer level:
//             2 s(parent) + parity, clamped to the inside centres, when the parent (ty >> 1, tx >> 1) lies in the coarser image,
//             was a target there and the result is in S; else the hashed pick.  Then one vote.
//   search    Jacobi: reads one NNF buffer and writes the other, so the result does not depend on the thread order.  Candidates
//             in a fixed order: s(t);  for st = 1, 2, 4 and d = (0,-st), (0,+st), (-st,0), (+st,0): s_old(t + d) - d if t + d is in
//             T;  s_best + (ry, rx), radius R = max(h, w), R / 2, ... >= 1 (k = 0, 1, ...), ry = (hash & 0xffff) % (2R + 1) - R,
//             rx = (hash >> 16) % (2R + 1) - R.  A candidate counts if it is in S and wins if its SSD is strictly smaller.
//   vote      a hole pixel p = (2 sum + n) / (2 n) of img[s(t) + (p - t)] over the n targets t whose patch covers p: a gather in
//             the fixed order of p - t, no atomics.  It reads known pixels only (S) and writes hole pixels only: in place.
//   schedule  per level: initial, vote, rounds x (iters searches, vote).  Fixed counts: nothing is read back inside.
//   output    known pixels bit for bit, hole pixels k / 255 in fp32; nnf [H, W, 2] = (sy, sx) or -1 off T; energy = the sum over T
//             of the SSD of (t, s(t)) on the final image (int64; an integer atomic per target, order-free).
//
// Shape: all levels of all images live in one workspace (level-major, image n of level l at lv.off + n hw).  The targets, the
// hole pixels and the sources of each (level, image) are compacted in raster order by csrc/compact_device.h's partition (1024
// consecutive pixels of ONE image per workgroup, ballot ranks, scan_kernel over the workgroups' totals), so the per-level
// launches are sized by the hole and not by the frame; the host reads the totals once, to size the lists and those launches.
// The search is one thread per target: its patch sits in registers (P is a template parameter, the loops are unrolled, no
// private array is indexed at run time), source patches are gathered from L2.  Per pixel the SSD is taken on the packed words
// as a.a + b.b - 2 a.b with the 4-way unsigned dot product (the a.a prefix per patch row is formed once per target), which
// needs no unpacking and no byte-wise difference; a candidate is dropped at the first check (every EXIT_ROWS rows) at which its
// partial sum reaches the best.  9 * 9 * 3 * 255^2 fits an int with room for the factor 2.
#include <algorithm>
#include <utility>
#include "compact_device.h"

namespace mvip {
namespace exemplar {

constexpr int BLOCK = 256;
constexpr int MAX_LEVELS = 8;
constexpr int MAX_SIDE = 16384;
constexpr int STATE = 32;                        // 32-bit words per image in meta, after the header
enum { S_LEVELS = 0, S_SINGULAR = 1, S_ENERGY = 2 /* and 3: one uint64 */, S_COUNT = 4 /* + 3 l + c */ };
// meta (int32 words): [0, 48) totals[l][c] as int64 (scan_kernel's), [48, 96) base[l][c] as int64: where list c of level l
// starts in `lists`, then STATE words per image.  c: 0 targets, 1 hole pixels, 2 sources.
constexpr int META_TOTALS = 0, META_BASE = 48, META_STATE = 96;
enum { F_HOLE = 1, F_BAD = 2, F_T = 4, F_S = 8 };
constexpr unsigned INIT_ITERATION = 0xffffffffu;
// a candidate's partial SSD is checked against the best after every EXIT_ROWS patch rows (and at the end).  The search is bound
// by the latency of its dependent gathers, not by arithmetic: a check after every row makes each row's loads wait for the
// previous row's verdict.  Measured on the fixture's 30 views, P = 7, per search launch: 1 row 36.5 us, 4 rows 26.6 us, no early
// exit 27.6 us.  The result does not depend on it.
#ifndef MVIP_EXEMPLAR_EXIT_ROWS
#define MVIP_EXEMPLAR_EXIT_ROWS 4
#endif
constexpr int EXIT_ROWS = MVIP_EXEMPLAR_EXIT_ROWS;

struct Level {
    int h, w, hw, G;                             // G: compaction workgroups per image
    long long off;                               // first pixel of the level in the per-pixel arrays
    long long goff;                              // first workgroup record of the level in wg
};
struct Shape {
    int N, P, L;
    Level lv[MAX_LEVELS];
    long long PX, GT;                            // pixels / workgroup records over all levels
};
struct Work {
    unsigned *img;                               // [PX] RGBX
    int *nnf0, *nnf1;                            // [PX] y w + x of the source, -1 off T
    int *wg;                                     // [GT * 3]
    unsigned char *flags, *rowf;                 // [PX]
};

__device__ __forceinline__ unsigned mix(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned key3(unsigned seed, int level, unsigned iteration) {
    return mix(mix(mix(seed ^ 0x9e3779b9u) + (unsigned)level) + iteration);
}
__device__ __forceinline__ unsigned hash2(unsigned key, unsigned k, unsigned pixel) { return mix(mix(key + k) + pixel); }
__device__ __forceinline__ const long long *totals_of(const int *meta) { return (const long long *)(meta + META_TOTALS); }
__device__ __forceinline__ const long long *bases_of(const int *meta) { return (const long long *)(meta + META_BASE); }

// ---- set-up -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void quantise_kernel(const float *__restrict__ v, const unsigned char *__restrict__ m,
                                                        const unsigned char *__restrict__ src, long long total, const Work w) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= total) return;
    const float a = v[3 * p], b = v[3 * p + 1], c = v[3 * p + 2];
    const bool hole = m[p] != 0 || !finite(a) || !finite(b) || !finite(c);
    unsigned word = 0;
    if (!hole) {
        const unsigned qa = (unsigned)rintf(fminf(fmaxf(a, 0.f), 1.f) * 255.f), qb = (unsigned)rintf(fminf(fmaxf(b, 0.f), 1.f) * 255.f),
                       qc = (unsigned)rintf(fminf(fmaxf(c, 0.f), 1.f) * 255.f);
        word = qa | (qb << 8) | (qc << 16);
    }
    w.img[p] = word;
    w.flags[p] = (hole ? F_HOLE | F_BAD : 0) | (src && !src[p] ? F_BAD : 0);
}

__global__ __launch_bounds__(BLOCK) void down_kernel(const Level f, const Level c, int N, const Work w) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (long long)N * c.hw) return;
    const int n = (int)(i / c.hw), p = (int)(i - (long long)n * c.hw), y = p / c.w, x = p - y * c.w;
    const long long fb = f.off + (long long)n * f.hw + (long long)(2 * y) * f.w + 2 * x;
    int cnt = 0, s0 = 0, s1 = 0, s2 = 0, fl = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long q = fb + (k >> 1) * f.w + (k & 1);
        const int g = w.flags[q];
        fl |= g & F_BAD;
        if (g & F_HOLE) continue;
        const unsigned word = w.img[q];
        ++cnt;
        s0 += word & 255;
        s1 += (word >> 8) & 255;
        s2 += (word >> 16) & 255;
    }
    unsigned word = 0;
    if (cnt) word = (unsigned)((2 * s0 + cnt) / (2 * cnt)) | ((unsigned)((2 * s1 + cnt) / (2 * cnt)) << 8) | ((unsigned)((2 * s2 + cnt) / (2 * cnt)) << 16);
    w.img[c.off + i] = word;
    w.flags[c.off + i] = (cnt < 4 ? F_HOLE | F_BAD : 0) | fl;
}

// the box test, row pass: at columns r .. w-1-r whether the 1 x P row segment holds a hole / a bad pixel
__global__ __launch_bounds__(BLOCK) void rowbox_kernel(const Level lv, int N, int r, const Work w) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (long long)N * lv.hw) return;
    const int x = (int)(i % lv.w);
    int f = 0;
    if (x >= r && x <= lv.w - 1 - r)
        for (int d = -r; d <= r; ++d) f |= w.flags[lv.off + i + d];
    w.rowf[lv.off + i] = (unsigned char)(f & (F_HOLE | F_BAD));
}
// column pass: T and S at the inside centres; both NNF buffers start as -1
__global__ __launch_bounds__(BLOCK) void colbox_kernel(const Level lv, int N, int r, const Work w) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (long long)N * lv.hw) return;
    const int p = (int)(i % lv.hw), y = p / lv.w, x = p - y * lv.w;
    int f = w.flags[lv.off + i] & (F_HOLE | F_BAD);
    if (y >= r && y <= lv.h - 1 - r && x >= r && x <= lv.w - 1 - r) {
        int g = 0;
        for (int d = -r; d <= r; ++d) g |= w.rowf[lv.off + i + (long long)d * lv.w];
        f |= (g & F_HOLE ? F_T : 0) | (g & F_BAD ? 0 : F_S);
    }
    w.flags[lv.off + i] = (unsigned char)f;
    w.nnf0[lv.off + i] = -1;
    w.nnf1[lv.off + i] = -1;
}

// compaction, first pass: workgroup (n, b) owns the pixels b * 1024 .. of image n; its three totals, and the image's counts
__device__ __forceinline__ int flag_of(int f, int c) { return c == 0 ? (f & F_T) != 0 : c == 1 ? (f & F_HOLE) != 0 : (f & F_S) != 0; }
__global__ __launch_bounds__(BLOCK) void count_kernel(const Level lv, int level, const Work w, int *__restrict__ meta) {
    __shared__ int tot[3];
    const int n = blockIdx.x / lv.G, b = blockIdx.x % lv.G;
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    int c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
    for (int q = 0; q < compact::PPT; ++q) {
        const int p = b * compact::PPB + q * BLOCK + threadIdx.x;
        const int f = p < lv.hw ? w.flags[lv.off + (long long)n * lv.hw + p] : 0;
        c0 += __popcll(__ballot(flag_of(f, 0)));
        c1 += __popcll(__ballot(flag_of(f, 1)));
        c2 += __popcll(__ballot(flag_of(f, 2)));
    }
    if (lane_id() == 0) {
        atomicAdd(&tot[0], c0);
        atomicAdd(&tot[1], c1);
        atomicAdd(&tot[2], c2);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        w.wg[(lv.goff + blockIdx.x) * 3 + threadIdx.x] = tot[threadIdx.x];
        if (tot[threadIdx.x]) atomicAdd(&meta[META_STATE + n * STATE + S_COUNT + 3 * level + threadIdx.x], tot[threadIdx.x]);
    }
}

// one thread: where each list starts; one thread per image: its level count
__global__ void plan_kernel(int N, int L, int *__restrict__ meta) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0) {
        const long long *tot = (const long long *)(meta + META_TOTALS);
        long long *base = (long long *)(meta + META_BASE), at = 0;
        for (int c = 0; c < 3; ++c)
            for (int l = 0; l < MAX_LEVELS; ++l) {
                base[3 * l + c] = at;
                at += l < L ? tot[3 * l + c] : 0;
            }
    }
    if (n >= N) return;
    int *st = meta + META_STATE + n * STATE;
    int levels = 0;
    while (levels < L && st[S_COUNT + 3 * levels + 2] > 0) ++levels;
    st[S_LEVELS] = levels;
    st[S_SINGULAR] = levels == 0;
}

// second pass: the lists, in raster order per image; an entry is n * hw + p
__global__ __launch_bounds__(BLOCK) void emit_kernel(const Level lv, int level, const Work w, const int *__restrict__ meta,
                                                    int *__restrict__ lists, long long capacity) {
    __shared__ int wtot[2][3][4];
    const int n = blockIdx.x / lv.G, b = blockIdx.x % lv.G;
    const long long *base = bases_of(meta);
    long long at[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) at[c] = base[3 * level + c] + w.wg[(lv.goff + blockIdx.x) * 3 + c];
#pragma unroll
    for (int q = 0; q < compact::PPT; ++q) {
        const int p = b * compact::PPB + q * BLOCK + threadIdx.x;
        const int f = p < lv.hw ? w.flags[lv.off + (long long)n * lv.hw + p] : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int keep = flag_of(f, c);
            int total;
            const int rank = compact::block_excl_small<1>(keep, wtot[q & 1][c], total);
            if (keep && at[c] + rank < capacity) lists[at[c] + rank] = n * lv.hw + p;
            at[c] += total;
        }
    }
}

// ---- one level -------------------------------------------------------------------------------------------------------------------
struct Item {
    int n, p, y, x;
    bool live;
};
// item idx of list c of this level; live: the image uses this level
__device__ __forceinline__ Item item(const Level &lv, int level, int c, const int *meta, const int *lists, int count) {
    Item it;
    it.live = false;
    it.n = it.p = it.y = it.x = 0;
    const long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= count || idx >= totals_of(meta)[3 * level + c]) return it;
    const int g = lists[bases_of(meta)[3 * level + c] + idx];
    it.n = g / lv.hw;
    it.p = g - it.n * lv.hw;
    it.y = it.p / lv.w;
    it.x = it.p - it.y * lv.w;
    it.live = level < meta[META_STATE + it.n * STATE + S_LEVELS];
    return it;
}

__global__ __launch_bounds__(BLOCK) void init_kernel(const Level lv, const Level par, int level, int r, unsigned seed, const Work w,
                                                    const int *__restrict__ parent_nnf, int *__restrict__ nnf,
                                                    const int *__restrict__ meta, const int *__restrict__ lists, int count) {
    const Item t = item(lv, level, 0, meta, lists, count);
    if (!t.live) return;
    const int *st = meta + META_STATE + t.n * STATE;
    const long long im = lv.off + (long long)t.n * lv.hw;
    int s = -1;
    if (level < st[S_LEVELS] - 1) {
        const int py = t.y >> 1, px = t.x >> 1;
        if (py < par.h && px < par.w) {
            const int ps = parent_nnf[par.off + (long long)t.n * par.hw + py * par.w + px];
            if (ps >= 0) {
                const int sy = min(max(2 * (ps / par.w) + (t.y & 1), r), lv.h - 1 - r), sx = min(max(2 * (ps % par.w) + (t.x & 1), r), lv.w - 1 - r);
                if (w.flags[im + sy * lv.w + sx] & F_S) s = sy * lv.w + sx;
            }
        }
    }
    if (s < 0) {
        const unsigned ns = (unsigned)st[S_COUNT + 3 * level + 2];
        const unsigned h = hash2(key3(seed, level, INIT_ITERATION), 0u, (unsigned)t.p);
        const long long first = bases_of(meta)[3 * level + 2] + w.wg[(lv.goff + (long long)t.n * lv.G) * 3 + 2];
        s = lists[first + h % ns] - t.n * lv.hw;
    }
    nnf[im + t.p] = s;
}

__global__ __launch_bounds__(BLOCK) void vote_kernel(const Level lv, int level, int r, const Work w, const int *__restrict__ nnf,
                                                    const int *__restrict__ meta, const int *__restrict__ lists, int count) {
    const Item q = item(lv, level, 1, meta, lists, count);
    if (!q.live) return;
    const long long im = lv.off + (long long)q.n * lv.hw;
    int cnt = 0, s0 = 0, s1 = 0, s2 = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const int ty = q.y - dy;
        if (ty < 0 || ty >= lv.h) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int tx = q.x - dx;
            if (tx < 0 || tx >= lv.w) continue;
            const int s = nnf[im + ty * lv.w + tx];
            if (s < 0) continue;
            const unsigned word = w.img[im + s + dy * lv.w + dx];
            ++cnt;
            s0 += word & 255;
            s1 += (word >> 8) & 255;
            s2 += (word >> 16) & 255;
        }
    }
    if (cnt) w.img[im + q.p] = (unsigned)((2 * s0 + cnt) / (2 * cnt)) | ((unsigned)((2 * s1 + cnt) / (2 * cnt)) << 8) | ((unsigned)((2 * s2 + cnt) / (2 * cnt)) << 16);
}

// the target's patch in registers, and the SSD against a source patch with an early exit per row
template <int P>
struct Patch {
    unsigned a[P * P];
    int aa[P];                                   // a.a over the rows 0 .. i
    __device__ __forceinline__ void load(const unsigned *img, int w, int y, int x) {
        constexpr int r = P / 2;
        int acc = 0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
#pragma unroll
            for (int j = 0; j < P; ++j) {
                a[i * P + j] = img[(y + i - r) * w + x + j - r];
                acc = (int)__builtin_amdgcn_udot4(a[i * P + j], a[i * P + j], (unsigned)acc, false);
            }
            aa[i] = acc;
        }
    }
    // the SSD if it is < best, else some value >= best
    __device__ __forceinline__ int ssd(const unsigned *img, int w, int sy, int sx, int best) const {
        constexpr int r = P / 2;
        const unsigned *b = img + (sy - r) * w + sx - r;
        unsigned bb = 0, ab = 0;
        int d = 0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const unsigned v = b[i * w + j];
                bb = __builtin_amdgcn_udot4(v, v, bb, false);
                ab = __builtin_amdgcn_udot4(a[i * P + j], v, ab, false);
            }
            if ((i + 1) % EXIT_ROWS == 0 || i == P - 1) {
                d = aa[i] + (int)bb - 2 * (int)ab;
                if (d >= best) return d;
            }
        }
        return d;
    }
};

template <int P>
__global__ __launch_bounds__(BLOCK) void search_kernel(const Level lv, int level, unsigned seed, unsigned iteration, const Work w,
                                                      const int *__restrict__ old, int *__restrict__ nnf,
                                                      const int *__restrict__ meta, const int *__restrict__ lists, int count) {
    constexpr int r = P / 2;
    const Item t = item(lv, level, 0, meta, lists, count);
    if (!t.live) return;
    const long long im = lv.off + (long long)t.n * lv.hw;
    const unsigned *img = w.img + im;
    const unsigned char *fl = w.flags + im;
    const int *on = old + im;
    Patch<P> patch;
    patch.load(img, lv.w, t.y, t.x);
    int cur = on[t.p];
    int best = patch.ssd(img, lv.w, cur / lv.w, cur % lv.w, 0x7fffffff);
    auto consider = [&](int cy, int cx) {
        if (cy < r || cy > lv.h - 1 - r || cx < r || cx > lv.w - 1 - r) return;
        if (!(fl[cy * lv.w + cx] & F_S)) return;
        const int d = patch.ssd(img, lv.w, cy, cx, best);
        if (d < best) {
            best = d;
            cur = cy * lv.w + cx;
        }
    };
    for (int st = 1; st <= 4; st <<= 1) {
        for (int k = 0; k < 4; ++k) {
            const int dy = k < 2 ? 0 : (k == 2 ? -st : st), dx = k >= 2 ? 0 : (k == 0 ? -st : st);
            const int qy = t.y + dy, qx = t.x + dx;
            if (qy < 0 || qy >= lv.h || qx < 0 || qx >= lv.w) continue;
            const int sq = on[qy * lv.w + qx];
            if (sq < 0) continue;
            consider(sq / lv.w - dy, sq % lv.w - dx);
        }
    }
    const unsigned key = key3(seed, level, iteration);
    unsigned k = 0;
    for (int R = max(lv.h, lv.w); R >= 1; R >>= 1, ++k) {
        const unsigned h = hash2(key, k, (unsigned)t.p);
        const int ry = (int)((h & 0xffffu) % (unsigned)(2 * R + 1)) - R, rx = (int)((h >> 16) % (unsigned)(2 * R + 1)) - R;
        consider(cur / lv.w + ry, cur % lv.w + rx);
    }
    nnf[im + t.p] = cur;
}

template <int P>
__global__ __launch_bounds__(BLOCK) void energy_kernel(const Level lv, const Work w, const int *__restrict__ nnf, int *__restrict__ meta,
                                                      const int *__restrict__ lists, int count) {
    const Item t = item(lv, 0, 0, meta, lists, count);
    if (!t.live) return;
    const long long im = lv.off + (long long)t.n * lv.hw;
    Patch<P> patch;
    patch.load(w.img + im, lv.w, t.y, t.x);
    const int s = nnf[im + t.p];
    const int d = patch.ssd(w.img + im, lv.w, s / lv.w, s % lv.w, 0x7fffffff);
    atomicAdd((unsigned long long *)(meta + META_STATE + t.n * STATE + S_ENERGY), (unsigned long long)d);
}

// ---- the end: known pixels bit for bit, hole pixels k / 255, the NNF as (sy, sx) ---------------------------------------------------
__global__ __launch_bounds__(BLOCK) void finish_kernel(const float *__restrict__ v, const Level lv, int N, const Work w,
                                                      const int *__restrict__ nnf, const int *__restrict__ meta,
                                                      float *__restrict__ out, int *__restrict__ nnf_out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (long long)N * lv.hw) return;
    const int n = (int)(i / lv.hw);
    const bool used = meta[META_STATE + n * STATE + S_LEVELS] > 0;
    float a = v[3 * i], b = v[3 * i + 1], c = v[3 * i + 2];
    if (used && (w.flags[i] & F_HOLE)) {
        const unsigned word = w.img[i];
        a = (float)(word & 255) / 255.f;
        b = (float)((word >> 8) & 255) / 255.f;
        c = (float)((word >> 16) & 255) / 255.f;
    }
    out[3 * i] = a;
    out[3 * i + 1] = b;
    out[3 * i + 2] = c;
    const int s = used ? nnf[i] : -1;
    nnf_out[2 * i] = s < 0 ? -1 : s / lv.w;
    nnf_out[2 * i + 1] = s < 0 ? -1 : s % lv.w;
}

}  // namespace exemplar
}  // namespace mvip

using namespace mvip;

static inline int64_t exemplar_align(int64_t b) { return (b + 255) / 256 * 256; }

// false: bad shape.  L levels (1 .. the geometric count) are laid out; every pixel and workgroup index must fit an int.
static inline bool exemplar_shape(int64_t N, int H, int W, int P, int L, exemplar::Shape &s) {
    if (N < 0 || N > INT32_MAX || H < 1 || W < 1 || H > exemplar::MAX_SIDE || W > exemplar::MAX_SIDE) return false;
    if (P < 3 || P > 9 || !(P & 1) || H < P || W < P || L < 1 || L > exemplar::MAX_LEVELS) return false;
    s.N = (int)N;
    s.P = P;
    s.L = L;
    s.PX = 0;
    s.GT = 0;
    int h = H, w = W;
    for (int l = 0; l < L; ++l) {
        if (l > 0) {
            if (std::min(h, w) / 2 < 4 * P) return false;
            h /= 2;
            w /= 2;
        }
        exemplar::Level &lv = s.lv[l];
        lv.h = h;
        lv.w = w;
        lv.hw = h * w;
        lv.G = (lv.hw + compact::PPB - 1) / compact::PPB;
        lv.off = s.PX;
        lv.goff = s.GT;
        s.PX += N * lv.hw;
        s.GT += N * lv.G;
    }
    return s.PX <= (int64_t)INT32_MAX / 4 && N <= (INT32_MAX - exemplar::META_STATE) / exemplar::STATE;
}
static inline exemplar::Work exemplar_carve(void *workspace, const exemplar::Shape &s) {
    char *c = (char *)workspace;
    exemplar::Work w;
    w.img = (unsigned *)c;             c += exemplar_align(s.PX * 4);
    w.nnf0 = (int *)c;                 c += exemplar_align(s.PX * 4);
    w.nnf1 = (int *)c;                 c += exemplar_align(s.PX * 4);
    w.wg = (int *)c;                   c += exemplar_align(s.GT * 12);
    w.flags = (unsigned char *)c;      c += exemplar_align(s.PX);
    w.rowf = (unsigned char *)c;
    return w;
}
// the buffer that holds a level's NNF after its schedule: the searches alternate, starting from nnf0
static inline int *exemplar_final_nnf(const exemplar::Work &w, int rounds, int iters) {
    return ((int64_t)rounds * iters) & 1 ? w.nnf1 : w.nnf0;
}

extern "C" int mvip_exemplar_levels(int H, int W, int patch, int max_levels) {
    if (H < 1 || W < 1 || H > exemplar::MAX_SIDE || W > exemplar::MAX_SIDE || patch < 3 || patch > 9 || !(patch & 1) || H < patch ||
        W < patch || max_levels < 0)
        return -1;
    const int cap = max_levels == 0 ? exemplar::MAX_LEVELS : std::min(max_levels, exemplar::MAX_LEVELS);
    int L = 1, h = H, w = W;
    while (L < cap && std::min(h, w) / 2 >= 4 * patch) {
        h /= 2;
        w /= 2;
        ++L;
    }
    return L;
}

extern "C" int64_t mvip_exemplar_meta_words(int64_t N) {
    if (N < 0 || N > (INT32_MAX - exemplar::META_STATE) / exemplar::STATE) return -1;
    return exemplar::META_STATE + N * exemplar::STATE;
}

extern "C" int64_t mvip_exemplar_workspace_bytes(int64_t N, int H, int W, int patch, int levels) {
    exemplar::Shape s;
    if (!exemplar_shape(N, H, W, patch, levels, s)) return -1;
    return 3 * exemplar_align(s.PX * 4) + exemplar_align(s.GT * 12) + 2 * exemplar_align(s.PX);
}

extern "C" int mvip_exemplar_setup(const float *images, const void *masks, const void *sources, int64_t N, int H, int W, int patch,
                                   int levels, void *workspace, int *meta, void *stream) {
    exemplar::Shape s;
    if (!exemplar_shape(N, H, W, patch, levels, s)) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!images || !masks || !workspace || !meta) return MVIP_EINVAL;
    const exemplar::Work w = exemplar_carve(workspace, s);
    hipStream_t st = as_stream(stream);
    const dim3 block(exemplar::BLOCK);
    zero_words(meta, (int)(exemplar::META_STATE + N * exemplar::STATE), st);
    hipLaunchKernelGGL(exemplar::quantise_kernel, dim3(blocks_for(N * s.lv[0].hw, exemplar::BLOCK)), block, 0, st, images,
                       (const unsigned char *)masks, (const unsigned char *)sources, (long long)(N * s.lv[0].hw), w);
    for (int l = 0; l < s.L; ++l) {
        const exemplar::Level &lv = s.lv[l];
        const dim3 grid(blocks_for(N * lv.hw, exemplar::BLOCK));
        if (l > 0) hipLaunchKernelGGL(exemplar::down_kernel, grid, block, 0, st, s.lv[l - 1], lv, s.N, w);
        hipLaunchKernelGGL(exemplar::rowbox_kernel, grid, block, 0, st, lv, s.N, patch / 2, w);
        hipLaunchKernelGGL(exemplar::colbox_kernel, grid, block, 0, st, lv, s.N, patch / 2, w);
        hipLaunchKernelGGL(exemplar::count_kernel, dim3((unsigned)(N * lv.G)), block, 0, st, lv, l, w, meta);
        hipLaunchKernelGGL((compact::scan_kernel<int, 3>), dim3(1), dim3(compact::SCAN_BLOCK), 0, st, w.wg + lv.goff * 3, (int)(N * lv.G),
                           (long long *)(meta + exemplar::META_TOTALS) + 3 * l);
    }
    hipLaunchKernelGGL(exemplar::plan_kernel, dim3(blocks_for(N, 64)), dim3(64), 0, st, s.N, s.L, meta);
    return check_launch();
}

extern "C" int mvip_exemplar_lists(int64_t N, int H, int W, int patch, int levels, void *workspace, const int *meta, int *lists,
                                   int64_t capacity, void *stream) {
    exemplar::Shape s;
    if (!exemplar_shape(N, H, W, patch, levels, s) || capacity < 0 || capacity > 3 * s.PX) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!workspace || !meta || !lists) return MVIP_EINVAL;
    const exemplar::Work w = exemplar_carve(workspace, s);
    for (int l = 0; l < s.L; ++l)
        hipLaunchKernelGGL(exemplar::emit_kernel, dim3((unsigned)(N * s.lv[l].G)), dim3(exemplar::BLOCK), 0, as_stream(stream), s.lv[l], l,
                           w, meta, lists, (long long)capacity);
    return check_launch();
}

template <int P>
static void exemplar_level_launch(const exemplar::Shape &s, int l, int64_t n_targets, int64_t n_holes, int rounds, int iters,
                                  unsigned seed, const exemplar::Work &w, int *meta, const int *lists, hipStream_t st) {
    const exemplar::Level &lv = s.lv[l], &par = s.lv[l + 1 < s.L ? l + 1 : l];
    const dim3 block(exemplar::BLOCK), gt(blocks_for(n_targets, exemplar::BLOCK)), gh(blocks_for(n_holes, exemplar::BLOCK));
    const int r = P / 2;
    int *cur = w.nnf0, *nxt = w.nnf1;
    hipLaunchKernelGGL(exemplar::init_kernel, gt, block, 0, st, lv, par, l, r, seed, w, (const int *)exemplar_final_nnf(w, rounds, iters),
                       cur, (const int *)meta, lists, (int)n_targets);
    hipLaunchKernelGGL(exemplar::vote_kernel, gh, block, 0, st, lv, l, r, w, (const int *)cur, (const int *)meta, lists, (int)n_holes);
    unsigned iteration = 0;
    for (int a = 0; a < rounds; ++a) {
        for (int b = 0; b < iters; ++b, ++iteration) {
            hipLaunchKernelGGL(exemplar::search_kernel<P>, gt, block, 0, st, lv, l, seed, iteration, w, (const int *)cur, nxt,
                               (const int *)meta, lists, (int)n_targets);
            std::swap(cur, nxt);
        }
        hipLaunchKernelGGL(exemplar::vote_kernel, gh, block, 0, st, lv, l, r, w, (const int *)cur, (const int *)meta, lists, (int)n_holes);
    }
    if (l == 0)
        hipLaunchKernelGGL(exemplar::energy_kernel<P>, gt, block, 0, st, lv, w, (const int *)cur, meta, lists, (int)n_targets);
}

extern "C" int mvip_exemplar_level(int64_t N, int H, int W, int patch, int levels, int level, int64_t n_targets, int64_t n_holes,
                                   int rounds, int iters, unsigned seed, void *workspace, int *meta, const int *lists, void *stream) {
    exemplar::Shape s;
    if (!exemplar_shape(N, H, W, patch, levels, s) || level < 0 || level >= levels || rounds < 0 || iters < 0 || n_targets < 0 ||
        n_holes < 0 || n_targets > N * s.lv[level].hw || n_holes > N * s.lv[level].hw || (n_targets == 0) != (n_holes == 0))
        return MVIP_EINVAL;
    if (N == 0 || n_targets == 0) return MVIP_OK;
    if (!workspace || !meta || !lists) return MVIP_EINVAL;
    const exemplar::Work w = exemplar_carve(workspace, s);
    hipStream_t st = as_stream(stream);
    switch (patch) {
        case 3: exemplar_level_launch<3>(s, level, n_targets, n_holes, rounds, iters, seed, w, meta, lists, st); break;
        case 5: exemplar_level_launch<5>(s, level, n_targets, n_holes, rounds, iters, seed, w, meta, lists, st); break;
        case 7: exemplar_level_launch<7>(s, level, n_targets, n_holes, rounds, iters, seed, w, meta, lists, st); break;
        default: exemplar_level_launch<9>(s, level, n_targets, n_holes, rounds, iters, seed, w, meta, lists, st); break;
    }
    return check_launch();
}

extern "C" int mvip_exemplar_finish(const float *images, int64_t N, int H, int W, int patch, int levels, int rounds, int iters,
                                    void *workspace, const int *meta, float *out, int *nnf, void *stream) {
    exemplar::Shape s;
    if (!exemplar_shape(N, H, W, patch, levels, s) || rounds < 0 || iters < 0) return MVIP_EINVAL;
    if (N == 0) return MVIP_OK;
    if (!images || !workspace || !meta || !out || !nnf || out == images) return MVIP_EINVAL;
    const exemplar::Work w = exemplar_carve(workspace, s);
    hipLaunchKernelGGL(exemplar::finish_kernel, dim3(blocks_for(N * s.lv[0].hw, exemplar::BLOCK)), dim3(exemplar::BLOCK), 0,
                       as_stream(stream), images, s.lv[0], s.N, w, (const int *)exemplar_final_nnf(w, rounds, iters), meta, out, nnf);
    return check_launch();
}
