// Connected components of a bit array (beyond the reference: it has no geometry clean-up): "keep the largest component",
// "drop components below N cells" for meshes (mvip_nerf_amd/mesh.py), occupancy grids and regions (mvip_nerf_amd/bitgrid.py).
//
// The array is [nx, ny, nz], z fastest, 1..768 per axis; element l = (i ny + j) nz + k is bit l & 31 of word l >> 5, tail bits
// zero: the layout of csrc/bitgrid_device.h, for cells and for the lattice points of csrc/mcubes.hip alike.
//
//   cc_pack:     fp32 values -> bits, bit l = values[l] >= threshold (NaN: clear; the "inside" of csrc/mcubes.hip).  One ballot
//                per 64 values = two words.
//   cc_init:     parent[l] = -1 for a clear bit, else the first element of the run of set bits that ends at l, as far as it can
//                be seen in l's own word and row.  Whole runs start out as one tree, so the z unions are left to the runs that
//                continue across a word boundary.
//   cc_union:    union-find over the set elements.  Every element unites itself with its set BACKWARD neighbours (3 at
//                connectivity 6, 13 at 26; a neighbour exists only inside the array): find both roots, atomicMin the lower into
//                the parent of the higher, and go on from what the atomic displaced until both sides meet.  A link always
//                points to a lower index, so a root is the lowest index of its tree and, at the end of the launch, of its
//                component whatever order the unions ran in: the result is reproducible though the route is not.
//                A union (l, nb) is skipped where l - 1 and nb - 1 are set too: l ~ l - 1 and nb ~ nb - 1 along z, and element
//                l - 1 makes (or in turn skips) the union (l - 1, nb - 1).  A solid block unites by its faces only.
//   cc_compress: parent[l] = root(l), and the roots of each workgroup counted for the compaction of csrc/compact_device.h
//                (items l with parent[l] == l); scan_kernel leaves n_components for the host, its one read.
//   cc_rank:     the emit pass: root l of rank r (ascending l, i.e. ascending lowest index of the components) writes
//                first[r] = l, sizes[r] = 0, labels[l] = r + 1; a clear bit writes label 0.
//   cc_assign:   labels[l] = labels[parent[l]] for the rest, sizes by integer atomicAdd (the two most frequent labels of a
//                wave added once per wave).  Integer sums do not depend on their order.
//   cc_select:   labels + keep table -> bits of the kept components, one ballot per 64 labels.
#include "bitgrid_device.h"
#include "compact_device.h"
#include "unionfind_device.h"

namespace mvip {
namespace cc {

using namespace bitgrid;
using namespace compact;
using namespace unionfind;             // load_parent, find, unite

constexpr int MAX_AXIS = 768;                // 3 * 768^3 < 2^31; the lattice limit of csrc/mcubes.hip

static inline bool axes_ok(int nx, int ny, int nz) {
    return nx >= 1 && nx <= MAX_AXIS && ny >= 1 && ny <= MAX_AXIS && nz >= 1 && nz <= MAX_AXIS;
}
static inline int64_t words_of(int64_t n) { return (n + 31) / 32; }

// the wave's 64 bits -> words 2 wv, 2 wv + 1 (wv = index of the wave's first element / 64); elements >= n carry 0
__device__ __forceinline__ void store_wave_bits(bool bit, int l, unsigned *__restrict__ words, int nwords) {
    const unsigned long long m = __ballot(bit);
    const int w0 = (l >> 6) * 2;
    if ((threadIdx.x & 63) == 0) {
        if (w0 < nwords) words[w0] = (unsigned)m;
        if (w0 + 1 < nwords) words[w0 + 1] = (unsigned)(m >> 32);
    }
}

__global__ __launch_bounds__(BLOCK) void cc_pack_kernel(const float *__restrict__ values, int n, float thr,
                                                       unsigned *__restrict__ words, int nwords) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    store_wave_bits(l < n && values[l] >= thr, l, words, nwords);
}

__global__ __launch_bounds__(BLOCK) void cc_init_kernel(const unsigned *__restrict__ words, int n, int nz,
                                                       int *__restrict__ parent) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= n) return;
    const unsigned w = words[l >> 5];
    const int b = l & 31;
    int p = -1;
    if ((w >> b) & 1u) {
        const unsigned clear_below = ~w & ((1u << b) - 1u);
        int run = clear_below ? b - 32 + __clz(clear_below) : b;     // set bits directly below b in this word
        const int k = l % nz;
        run = run < k ? run : k;                                       // ... that belong to this row
        p = l - run;
    }
    parent[l] = p;
}

template <int CONN>
__global__ __launch_bounds__(BLOCK) void cc_union_kernel(const unsigned *__restrict__ words, int nx, int ny, int nz,
                                                        int *parent) {
    const int n = nx * ny * nz;
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= n || !cell_bit(words, l)) return;
    int i, j, k;
    linear_ijk(l, ny, nz, i, j, k);
    const bool prev = k > 0 && cell_bit(words, l - 1);
    if (prev && (l & 31) == 0) unite(parent, l, l - 1);      // inside a word cc_init has made the tie
#pragma unroll
    for (int di = -1; di <= 0; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
            for (int dk = -1; dk <= 1; ++dk) {
                const bool backward = di < 0 || (di == 0 && dj < 0);             // (0, 0, -1) is the case above
                const bool face = (di != 0) + (dj != 0) + (dk != 0) == 1;
                if (!backward || (CONN == 6 && !face)) continue;
                const int x = i + di, y = j + dj, z = k + dk;
                if (x < 0 || y < 0 || y >= ny || z < 0 || z >= nz) continue;
                const int nb = (x * ny + y) * nz + z;
                if (!cell_bit(words, nb)) continue;
                if (prev && z > 0 && cell_bit(words, nb - 1)) continue;          // element l - 1 ties the two runs
                unite(parent, l, nb);
            }
}

__global__ __launch_bounds__(BLOCK) void cc_compress_kernel(int *parent, int n, int *__restrict__ wg_sums) {
    __shared__ int wtot[4];
    int sum = 0;
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int l = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        bool root = false;
        if (l < n) {
            const int p = load_parent(parent, l);
            if (p >= 0) {
                const int r = find(parent, p);
                if (r != p) __hip_atomic_store(parent + l, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                root = r == l;
            }
        }
        int wt;
        wave_excl_small<1>(root, wt);
        sum += wt;
    }
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) wg_sums[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

__global__ __launch_bounds__(BLOCK) void cc_rank_kernel(const int *__restrict__ parent, int n, const int *__restrict__ wg_off,
                                                       int nc, int *__restrict__ labels, int *__restrict__ sizes,
                                                       int *__restrict__ first) {
    __shared__ int wtot[2][4];
    int base = wg_off[blockIdx.x];
#pragma unroll
    for (int q = 0; q < PPT; ++q) {
        const int l = blockIdx.x * PPB + q * BLOCK + threadIdx.x;
        const int p = l < n ? parent[l] : -1;
        const bool root = p == l;                            // l >= 0 > -1: never for a clear bit or past the end
        int total;
        const int id = base + block_excl_small<1>(root, wtot[q & 1], total);
        if (root && id < nc) {
            first[id] = l;
            sizes[id] = 0;
            labels[l] = id + 1;
        } else if (l < n && p < 0) {
            labels[l] = 0;
        }
        base += total;
    }
}

// labels: the roots' entries are read, the other set elements' entries written (no __restrict__)
__global__ __launch_bounds__(BLOCK) void cc_assign_kernel(const int *__restrict__ parent, int n, int nc, int *labels,
                                                         int *__restrict__ sizes) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    const int p = l < n ? parent[l] : -1;
    int lab = 0;
    if (p >= 0) {
        lab = labels[p];
        if (p != l) labels[l] = lab;
    }
    bool pending = lab > 0 && lab <= nc;
#pragma unroll
    for (int round = 0; round < 2; ++round) {                // the wave's leading labels: one atomic each
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) break;
        const int leader = __ffsll((long long)m) - 1;
        const int ll = __shfl(lab, leader, 64);
        const bool same = pending && lab == ll;
        const unsigned long long sm = __ballot(same);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(sizes + (ll - 1), (int)__popcll(sm));
        pending = pending && !same;
    }
    if (pending) atomicAdd(sizes + (lab - 1), 1);
}

__global__ __launch_bounds__(BLOCK) void cc_select_kernel(const int *__restrict__ labels, int n,
                                                         const unsigned char *__restrict__ keep, int nc,
                                                         unsigned *__restrict__ words, int nwords) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    bool bit = false;
    if (l < n) {
        const int lab = labels[l];
        bit = lab > 0 && lab <= nc && keep[lab] != 0;
    }
    store_wave_bits(bit, l, words, nwords);
}

}  // namespace cc
}  // namespace mvip

using namespace mvip;

static const int64_t CC_MAX_N = (int64_t)cc::MAX_AXIS * cc::MAX_AXIS * cc::MAX_AXIS;

extern "C" int mvip_components_pack(const float *values, int64_t n, float threshold, int *words, void *stream) {
    if (n < 0 || n > CC_MAX_N || threshold != threshold) return MVIP_EINVAL;
    if (n == 0) return MVIP_OK;
    if (!values || !words) return MVIP_EINVAL;
    hipLaunchKernelGGL(cc::cc_pack_kernel, dim3(blocks_for(n, cc::BLOCK)), dim3(cc::BLOCK), 0, as_stream(stream), values, (int)n,
                       threshold, (unsigned *)words, (int)cc::words_of(n));
    return check_launch();
}

extern "C" int64_t mvip_components_groups(int nx, int ny, int nz) {
    if (!cc::axes_ok(nx, ny, nz)) return -1;
    return ((int64_t)nx * ny * nz + cc::PPB - 1) / cc::PPB;
}

extern "C" int mvip_components_label(const int *words, int nx, int ny, int nz, int connectivity, int *parent, int *wg,
                                     int64_t *total, void *stream) {
    const int64_t G = mvip_components_groups(nx, ny, nz);
    if (G < 0 || (connectivity != 6 && connectivity != 26)) return MVIP_EINVAL;
    if (!words || !parent || !wg || !total) return MVIP_EINVAL;
    const int n = nx * ny * nz;
    const dim3 grid(blocks_for(n, cc::BLOCK)), block(cc::BLOCK);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(cc::cc_init_kernel, grid, block, 0, s, (const unsigned *)words, n, nz, parent);
    if (connectivity == 6)
        hipLaunchKernelGGL(cc::cc_union_kernel<6>, grid, block, 0, s, (const unsigned *)words, nx, ny, nz, parent);
    else
        hipLaunchKernelGGL(cc::cc_union_kernel<26>, grid, block, 0, s, (const unsigned *)words, nx, ny, nz, parent);
    hipLaunchKernelGGL(cc::cc_compress_kernel, dim3((unsigned)G), block, 0, s, parent, n, wg);
    hipLaunchKernelGGL((compact::scan_kernel<int, 1>), dim3(1), dim3(compact::SCAN_BLOCK), 0, s, wg, (int)G,
                       (long long *)total);
    return check_launch();
}

extern "C" int mvip_components_rank(const int *parent, int nx, int ny, int nz, const int *wg, int64_t n_components,
                                    int *labels, int *sizes, int *first, void *stream) {
    const int64_t G = mvip_components_groups(nx, ny, nz);
    if (G < 0 || n_components < 0 || n_components > (int64_t)nx * ny * nz) return MVIP_EINVAL;
    if (n_components == 0) return MVIP_OK;
    if (!parent || !wg || !labels || !sizes || !first) return MVIP_EINVAL;
    const int n = nx * ny * nz;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(cc::cc_rank_kernel, dim3((unsigned)G), dim3(cc::BLOCK), 0, s, parent, n, wg, (int)n_components, labels,
                       sizes, first);
    hipLaunchKernelGGL(cc::cc_assign_kernel, dim3(blocks_for(n, cc::BLOCK)), dim3(cc::BLOCK), 0, s, parent, n,
                       (int)n_components, labels, sizes);
    return check_launch();
}

extern "C" int mvip_components_select(const int *labels, int64_t n, const void *keep, int64_t n_components, int *words,
                                      void *stream) {
    if (n < 0 || n > CC_MAX_N || n_components < 0 || n_components > n) return MVIP_EINVAL;
    if (n == 0) return MVIP_OK;
    if (!labels || !keep || !words) return MVIP_EINVAL;
    hipLaunchKernelGGL(cc::cc_select_kernel, dim3(blocks_for(n, cc::BLOCK)), dim3(cc::BLOCK), 0, as_stream(stream), labels,
                       (int)n, (const unsigned char *)keep, (int)n_components, (unsigned *)words, (int)cc::words_of(n));
    return check_launch();
}
