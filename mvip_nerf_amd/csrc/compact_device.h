// Order-preserving compaction of a long run of items, each emitting a small count of outputs (csrc/mcubes.hip: 0..3 vertices
// and 0..5 triangles per lattice point; csrc/occupancy.hip: 0..1 kept samples per sample).
//
// Every pass partitions the items the same way: workgroup b owns the PPB = 1024 consecutive items starting at b * PPB, thread
// t of it the items b * PPB + q * 256 + t, q = 0..3 (coalesced).  Within a round q a count is ranked in item order on the
// wave's ballot masks (v_mbcnt per bit plane of the count) plus four wave totals in LDS (two buffers in turn: one barrier
// per round).  A first pass writes the workgroups' totals, scan_kernel turns them into exclusive offsets in place and leaves
// the grand totals for the host (its one read, to allocate the outputs), the emit pass adds offset + rank.  No atomics: the
// output order is the item order and the result is reproducible bit for bit.
#pragma once
#include "common.h"

namespace mvip {
namespace compact {

constexpr int BLOCK = 256;
constexpr int PPT = 4;                       // items per thread
constexpr int PPB = BLOCK * PPT;             // items per workgroup
constexpr int SCAN_BLOCK = 1024;
constexpr int SCAN_PER_THREAD = 8;

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// exclusive prefix across the wave of a count in 0 .. 2^BITS - 1, from its bit planes; `total` = the wave's sum
template <int BITS>
__device__ __forceinline__ int wave_excl_small(int c, int &total) {
    int pre = 0;
    total = 0;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const unsigned long long m = __ballot((c >> b) & 1);
        pre += lanes_below(m) << b;
        total += __popcll(m) << b;
    }
    return pre;
}

// exclusive prefix across the workgroup (4 waves, lane order = item order); `total` = the workgroup's sum.
// wtot: 4 LDS words of this call's buffer (callers alternate two buffers, so one barrier per call suffices).
template <int BITS>
__device__ __forceinline__ int block_excl_small(int c, int *wtot, int &total) {
    const int w = threadIdx.x >> 6;
    int wt;
    const int pre = wave_excl_small<BITS>(c, wt);
    if ((threadIdx.x & 63) == 0) wtot[w] = wt;
    __syncthreads();
    const int t0 = wtot[0], t1 = wtot[1], t2 = wtot[2], t3 = wtot[3];
    total = t0 + t1 + t2 + t3;
    return pre + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
}

template <class T>
__device__ __forceinline__ T wave_incl(T x) {
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (l >= o) x += y;
    }
    return x;
}

// in-place exclusive scan of G records of W interleaved counters (wg [G, W]); totals[0 .. W - 1] = their sums.  One
// workgroup of 1024 threads, each thread owning SCAN_PER_THREAD consecutive records of an 8192-record chunk; the chunks in
// turn, the sums so far carried along.
template <class T, int W>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_kernel(T *__restrict__ wg, int G, long long *__restrict__ totals) {
    __shared__ T wsum[2][SCAN_BLOCK / 64][W];
    T carry[W];
#pragma unroll
    for (int c = 0; c < W; ++c) carry[c] = 0;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    int buf = 0;
    for (int c0 = 0; c0 < G; c0 += SCAN_BLOCK * SCAN_PER_THREAD) {
        const int g0 = c0 + threadIdx.x * SCAN_PER_THREAD;
        T own[W], incl[W], ev[W], tot[W];
#pragma unroll
        for (int c = 0; c < W; ++c) own[c] = 0;
        for (int e = 0; e < SCAN_PER_THREAD; ++e)
            if (g0 + e < G) {
#pragma unroll
                for (int c = 0; c < W; ++c) own[c] += wg[W * (g0 + e) + c];
            }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            incl[c] = wave_incl(own[c]);
            if (l == 63) wsum[buf][w][c] = incl[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < W; ++c) {
            T below = 0;
            tot[c] = 0;
            for (int u = 0; u < SCAN_BLOCK / 64; ++u) {
                const T a = wsum[buf][u][c];
                if (u < w) below += a;
                tot[c] += a;
            }
            ev[c] = carry[c] + below + incl[c] - own[c];
        }
        for (int e = 0; e < SCAN_PER_THREAD; ++e)
            if (g0 + e < G) {
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const T a = wg[W * (g0 + e) + c];
                    wg[W * (g0 + e) + c] = ev[c];
                    ev[c] += a;
                }
            }
#pragma unroll
        for (int c = 0; c < W; ++c) carry[c] += tot[c];
        buf ^= 1;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < W; ++c) totals[c] = carry[c];
    }
}

}  // namespace compact
}  // namespace mvip
