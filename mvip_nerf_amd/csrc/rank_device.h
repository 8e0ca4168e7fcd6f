// Ranks of small counts over a long run of items, on the partition of compact_device.h: rank[i] = sum of count(i') over
// i' < i, the grand total left for the host.  Shared by the mesh clean-up (csrc/mesh_ops.hip: cluster ids, kept faces,
// referenced clusters) and the mesh topology (csrc/mesh_topology.hip: edge ids, component and loop numbers, cap outputs).
// `count` is any functor int -> 0 .. 2^BITS - 1.  wg: one int32 word per workgroup of PPB items (mvip_mesh_rank_groups).
#pragma once
#include "compact_device.h"

namespace mvip {
namespace compact {

struct Flag {
    const int *f;
    __device__ __forceinline__ int operator()(int i) const { return f[i] != 0; }
};

template <class C, int BITS>
__global__ __launch_bounds__(BLOCK) void rank_count_kernel(C count, int n, int *__restrict__ wg_sums) {
    __shared__ int wtot[4];
    int sum = 0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int i = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        int wt;
        wave_excl_small<BITS>(i < n ? count(i) : 0, wt);
        sum += wt;
    }
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) wg_sums[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

template <class C, int BITS>
__global__ __launch_bounds__(BLOCK) void rank_emit_kernel(C count, int n, const int *__restrict__ wg_off, int *__restrict__ rank) {
    __shared__ int wtot[2][4];
    int base = wg_off[blockIdx.x];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int i = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        int total;
        const int r = base + block_excl_small<BITS>(i < n ? count(i) : 0, wtot[q & 1], total);
        if (i < n) rank[i] = r;
        base += total;
    }
}

template <class C, int BITS>
static void ranks(C count, int n, int *wg, int64_t *total, int *rank, hipStream_t s) {
    const unsigned G = blocks_for(n, PPB);                     // n == 0: the scan alone, which leaves total = 0
    if (G) hipLaunchKernelGGL((rank_count_kernel<C, BITS>), dim3(G), dim3(BLOCK), 0, s, count, n, wg);
    hipLaunchKernelGGL((scan_kernel<int, 1>), dim3(1), dim3(SCAN_BLOCK), 0, s, wg, (int)G, (long long *)total);
    if (G) hipLaunchKernelGGL((rank_emit_kernel<C, BITS>), dim3(G), dim3(BLOCK), 0, s, count, n, (const int *)wg, rank);
}

}  // namespace compact
}  // namespace mvip
