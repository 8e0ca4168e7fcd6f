// Topology of an indexed triangle mesh (beyond the reference, which has no mesh export at all): the edge table, the face
// components, the boundary loops and a centroid-fan cap of the small ones (ops.mesh_edge_table / mesh_components /
// mesh_boundary_loops / mesh_cap_loops, mvip_nerf_amd/mesh.py: topology, keep_components, boundary_loops, close_holes).
// THE statement of the definitions; restated for the tests in tests/mesh_topology_numpy.py.
//
// verts [V, 3] fp32, faces [F, 3] int32: the conventions of csrc/mesh_ops.hip.  Half-edge h = 3 f + k runs from
// a = faces[f, k] (its origin; corner h of the corner table) to b = faces[f, (k + 1) % 3].  A face that names a vertex twice is
// DEGENERATE and takes no part in anything below: edge_of = -1, label 0, never a boundary.  A face index outside [0, V) raises
// a flag (the caller's ValueError); such a face is treated as degenerate so that no kernel reads out of bounds.
//
// EDGE TABLE.  Two half-edges of non-degenerate faces belong to one edge iff their unordered endpoints (lo, hi) are equal.  The
// lists of csrc/mesh_ops.hip are built over keys = lo of every half-edge (-1: left out), K = V; one thread per half-edge walks
// the list of its own lo and finds the REPRESENTATIVE of its edge (the lowest half-edge of the edge: the first of the ascending
// list with the same hi), count (the half-edges of the edge) and forward (those of them that run lo -> hi).  Edge ids are the
// ranks of the representatives in ascending half-edge order (rank_device.h); E is the one read-back.  edge_of [3F], edges
// [E, 2] = (lo, hi), first [E] the representative, count [E], forward [E], twin [3F] = the other half-edge of an edge with
// exactly two, else -1.  Classes: boundary count == 1; interior count == 2 and forward == 1; inconsistent count == 2 and
// forward != 1; non-manifold count >= 3.  The walk is QUADRATIC in the valence (every half-edge of a vertex's lo-list walks
// the whole list), as list_rank_kernel is: a vertex shared by n faces costs n^2 steps, which is nothing at the valence 6 of a
// marching-cubes mesh and is the price of a 10^5-triangle fan.
//
// FACE COMPONENTS.  Union-find over face indices (unionfind_device.h: atomicMin towards the lower index; parent[x] <= x, so
// every walk ends).  'edge': every half-edge unites its face with its representative's face.  'vertex': every corner of a
// non-degenerate face unites its face with the face of the first corner of its vertex's corner list that belongs to a
// non-degenerate face.  Compress; the roots (each the lowest face of its component) are ranked in ascending order: labels are
// 1..C in order of each component's lowest face, 0 for degenerate faces (the convention of csrc/components.hip); C is the one
// read-back.  table [C, 6] int32 by integer atomicAdd (the order of arrival does not matter):
//   0 faces;  1 vertices: a corner counts iff its face's label is not 0 and no EARLIER corner of its vertex's corner list has
//   the same label (a vertex counts once per component present in its list);  2 edges, by the label of the representative's
//   face;  3 boundary,  4 non-manifold,  5 inconsistent edges, likewise.
//
// BOUNDARY LOOPS.  A boundary half-edge is the only half-edge of its edge.  For a boundary half-edge h: a -> b, next[h] = the
// boundary half-edge that starts at b, if exactly one boundary half-edge starts at b (read from b's corner list: corner c is
// the origin of half-edge c) and exactly one ends there (an integer count per vertex); else -1, as for every other half-edge.
// Loops are the components of h ~ next[h] (the same union-find over half-edge indices), ranked by their lowest half-edge; L is
// the one read-back.  loop_of [3F] (-1 off the boundary), first [L], sizes [L], closed [L] = 1 iff every member has a next.
// A closed loop is a simple cycle: next is injective (two half-edges with one next would both end at its origin, where
// exactly one ends), so on the finite set of the loop's members, each of which has a next inside the loop, it is a
// permutation, and a connected permutation is one cycle; it visits a vertex once because only one boundary half-edge starts
// at any of its vertices.
//
// CAPS.  A loop is capped iff closed and 3 <= size <= max_edges.  The lists again, keys = the loop of every half-edge of a
// capped loop (so no list is longer than max_edges), K = L.  Per capped loop (one thread) over its ascending list: the new
// vertex = (fp64 sum of the fp32 origin vertices, front to back) / n, rounded once to fp32; the colour = (2 sum + n) / (2 n)
// in integers, as in csrc/mesh_ops.hip.  Per half-edge h: a -> b of a capped loop the new face (b, a, V + cap number):
// reversed, so that a consistently oriented mesh stays so.  New faces come out in ascending half-edge order, new vertices in
// loop order (both through the order-preserving ranks).
//
// No float atomics, no LDS beyond compact_device.h's, no scratch.  Every loop runs over one list (trip count = its length)
// or is a union-find walk (bounded by parent[x] <= x).
#include "compact_device.h"
#include "rank_device.h"
#include "unionfind_device.h"

namespace mvip {
namespace meshtopo {

using namespace compact;
using namespace unionfind;

static const int64_t INT_MAX64 = 2147483647;

struct IsOwn {                               // rep[i] == i: representatives
    const int *rep;
    __device__ __forceinline__ int operator()(int i) const { return rep[i] == i; }
};
struct NonNegative {
    const int *k;
    __device__ __forceinline__ int operator()(int i) const { return k[i] >= 0; }
};

__global__ __launch_bounds__(BLOCK) void fill_kernel(int *__restrict__ p, int n, int value) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) p[i] = value;
}

// the destination corner of half-edge h
__device__ __forceinline__ int head_of(int h) {
    const int f = h / 3, k = h - 3 * f;
    return k == 2 ? 3 * f : h + 1;
}

// +1 on counter[stride * lab] for every lane with `pending`; the wave's two leading labels are added once per wave (a mesh
// is mostly one component).  Every lane of the wave must make the call.  Integer sums do not depend on their order.
__device__ __forceinline__ void count_label(int *counter, int stride, int lab, bool pending) {
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) break;
        const int leader = __ffsll((long long)m) - 1;
        const int ll = __shfl(lab, leader, 64);
        const bool same = pending && lab == ll;
        const unsigned long long sm = __ballot(same);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(counter + (int64_t)stride * ll, (int)__popcll(sm));
        pending = pending && !same;
    }
    if (pending) atomicAdd(counter + (int64_t)stride * lab, 1);
}

// ---- edge table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void keys_kernel(const int *__restrict__ faces, int n, int V, int *__restrict__ keys,
                                                    int *flag) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int f = h / 3;
    const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    int key = -1;
    if ((unsigned)v0 >= (unsigned)V || (unsigned)v1 >= (unsigned)V || (unsigned)v2 >= (unsigned)V) {
        atomicOr(flag, 1);
    } else if (v0 != v1 && v1 != v2 && v0 != v2) {
        const int a = faces[h], b = faces[head_of(h)];
        key = a < b ? a : b;
    }
    keys[h] = key;
}

__global__ __launch_bounds__(BLOCK) void edge_find_kernel(const int *__restrict__ faces, int n, const int *__restrict__ keys,
                                                         const int *__restrict__ offsets, const int *__restrict__ items,
                                                         int *__restrict__ rep, int *__restrict__ hcount,
                                                         int *__restrict__ hforward, int *__restrict__ twin) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int lo = keys[h];
    int r = -1, cnt = 0, fwd = 0, other = -1;
    if (lo >= 0) {
        const int a = faces[h], b = faces[head_of(h)];
        const int hi = a == lo ? b : a;
        const int end = offsets[lo + 1];
        for (int j = offsets[lo]; j < end; ++j) {            // the half-edges whose lower endpoint is lo, ascending
            const int g = items[j];
            const int ga = faces[g], gb = faces[head_of(g)];
            if ((ga == lo ? gb : ga) != hi) continue;
            if (r < 0) r = g;
            ++cnt;
            fwd += ga == lo;
            if (g != h) other = g;
        }
    }
    rep[h] = r;
    hcount[h] = cnt;
    hforward[h] = fwd;
    twin[h] = cnt == 2 ? other : -1;
}

__global__ __launch_bounds__(BLOCK) void edge_emit_kernel(const int *__restrict__ faces, int n, const int *__restrict__ rep,
                                                         const int *__restrict__ hcount, const int *__restrict__ hforward,
                                                         const int *__restrict__ rank, int E, int *__restrict__ edge_of,
                                                         int *__restrict__ edges, int *__restrict__ first,
                                                         int *__restrict__ count, int *__restrict__ forward) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int r = rep[h];
    edge_of[h] = r < 0 ? -1 : rank[r];
    if (r != h) return;
    const int e = rank[h];
    if (e >= E) return;
    const int a = faces[h], b = faces[head_of(h)];
    edges[2 * e] = a < b ? a : b;
    edges[2 * e + 1] = a < b ? b : a;
    first[e] = h;
    count[e] = hcount[h];
    forward[e] = hforward[h];
}

// ---- union-find plumbing ------------------------------------------------------------------------------------------------
// parent[l] = root(l), is_root[l] = (root(l) == l); elements with parent -1 take no part.  Runs after the launch that united.
__global__ __launch_bounds__(BLOCK) void compress_kernel(int *parent, int n, int *__restrict__ is_root) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= n) return;
    const int p = load_parent(parent, l);
    int root = 0;
    if (p >= 0) {
        const int r = find(parent, p);
        if (r != p) __hip_atomic_store(parent + l, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        root = r == l;
    }
    is_root[l] = root;
}

// ---- face components ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void face_init_kernel(const int *__restrict__ rep, int F, int *__restrict__ parent) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    if (f < F) parent[f] = rep[3 * f] < 0 ? -1 : f;          // rep < 0: a degenerate face
}

__global__ __launch_bounds__(BLOCK) void face_union_edge_kernel(const int *__restrict__ rep, int n, int *parent) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int r = rep[h];
    if (r < 0 || r == h) return;
    const int f = h / 3, g = r / 3;
    if (f != g) unite(parent, f, g);
}

__global__ __launch_bounds__(BLOCK) void face_union_vertex_kernel(const int *__restrict__ faces, int n, int V,
                                                                 const int *__restrict__ rep, const int *__restrict__ offsets,
                                                                 const int *__restrict__ corners, int *parent) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n) return;
    const int f = c / 3;
    if (rep[3 * f] < 0) return;
    const int v = faces[c];
    if ((unsigned)v >= (unsigned)V) return;                  // never: rep >= 0 says the face's indices are inside
    const int end = offsets[v + 1];
    for (int j = offsets[v]; j < end; ++j) {                 // the first corner of v that belongs to a non-degenerate face
        const int g = corners[j] / 3;
        if (rep[3 * g] < 0) continue;
        if (g != f) unite(parent, f, g);
        break;
    }
}

__global__ __launch_bounds__(BLOCK) void face_label_kernel(const int *__restrict__ parent, int F, const int *__restrict__ rank,
                                                          int C, int *__restrict__ labels, int *table) {
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    int lab = 0;
    if (f < F) {
        const int p = parent[f];
        lab = p < 0 ? 0 : rank[p] + 1;
        labels[f] = lab;
    }
    count_label(table + 0, 6, lab - 1, lab > 0 && lab <= C);
}

// position j of the corner table: the corner counts iff no earlier corner of the same list has its label
__global__ __launch_bounds__(BLOCK) void vertex_count_kernel(const int *__restrict__ faces, int n, int V,
                                                            const int *__restrict__ offsets, const int *__restrict__ corners,
                                                            const int *__restrict__ labels, int C, int *table) {
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    int lab = 0;
    bool counts = false;
    if (j < n) {
        const int c = corners[j];
        lab = labels[c / 3];
        const int v = faces[c];
        if (lab > 0 && lab <= C && (unsigned)v < (unsigned)V) {
            counts = true;
            for (int u = offsets[v]; u < j; ++u)
                if (labels[corners[u] / 3] == lab) {
                    counts = false;
                    break;
                }
        }
    }
    count_label(table + 1, 6, lab - 1, counts);
}

__global__ __launch_bounds__(BLOCK) void edge_count_kernel(int n, const int *__restrict__ rep, const int *__restrict__ hcount,
                                                          const int *__restrict__ hforward, const int *__restrict__ labels,
                                                          int C, int *table) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    int lab = 0, cnt = 0, fwd = 0;
    bool own = false;
    if (h < n && rep[h] == h) {
        lab = labels[h / 3];
        own = lab > 0 && lab <= C;
        cnt = hcount[h];
        fwd = hforward[h];
    }
    count_label(table + 2, 6, lab - 1, own);
    count_label(table + 3, 6, lab - 1, own && cnt == 1);
    count_label(table + 4, 6, lab - 1, own && cnt >= 3);
    count_label(table + 5, 6, lab - 1, own && cnt == 2 && fwd != 1);
}

// ---- boundary loops -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_boundary(const int *__restrict__ rep, const int *__restrict__ hcount, int h) {
    return rep[h] == h && hcount[h] == 1;
}

__global__ __launch_bounds__(BLOCK) void loop_ends_kernel(const int *__restrict__ faces, int n, int V, const int *__restrict__ rep,
                                                         const int *__restrict__ hcount, int *ends) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n || !is_boundary(rep, hcount, h)) return;
    const int b = faces[head_of(h)];
    if ((unsigned)b < (unsigned)V) atomicAdd(ends + b, 1);
}

__global__ __launch_bounds__(BLOCK) void loop_next_kernel(const int *__restrict__ faces, int n, int V, const int *__restrict__ rep,
                                                         const int *__restrict__ hcount, const int *__restrict__ offsets,
                                                         const int *__restrict__ corners, const int *__restrict__ ends,
                                                         int *__restrict__ next, int *__restrict__ parent) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    int nx = -1, p = -1;
    if (is_boundary(rep, hcount, h)) {
        p = h;
        const int b = faces[head_of(h)];
        if ((unsigned)b < (unsigned)V && ends[b] == 1) {
            int starts = 0, cand = -1;
            const int end = offsets[b + 1];
            for (int j = offsets[b]; j < end; ++j) {         // corner c of b is the origin of half-edge c
                const int c = corners[j];
                if (is_boundary(rep, hcount, c)) {
                    ++starts;
                    cand = c;
                }
            }
            if (starts == 1) nx = cand;
        }
    }
    next[h] = nx;
    parent[h] = p;
}

__global__ __launch_bounds__(BLOCK) void loop_union_kernel(const int *__restrict__ next, int n, int *parent) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int nx = next[h];
    if (nx >= 0 && nx != h) unite(parent, h, nx);
}

__global__ __launch_bounds__(BLOCK) void loop_emit_kernel(const int *__restrict__ parent, int n, const int *__restrict__ rank,
                                                         const int *__restrict__ next, int L, int *__restrict__ loop_of,
                                                         int *__restrict__ first, int *sizes, int *closed) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    int l = -1;
    if (h < n) {
        const int p = parent[h];
        l = p < 0 ? -1 : rank[p];
        if (l >= L) l = -1;                                  // never
        loop_of[h] = l;
        if (l >= 0) {
            if (p == h) first[l] = h;
            if (next[h] < 0) atomicAnd(closed + l, 0);
        }
    }
    count_label(sizes, 1, l, l >= 0);
}

// ---- caps ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void cap_choose_kernel(const int *__restrict__ sizes, const int *__restrict__ closed, int L,
                                                          int max_edges, int *__restrict__ capped) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l < L) capped[l] = closed[l] != 0 && sizes[l] >= 3 && sizes[l] <= max_edges;
}

__global__ __launch_bounds__(BLOCK) void cap_keys_kernel(const int *__restrict__ loop_of, int n, int L,
                                                        const int *__restrict__ capped, int *__restrict__ keys) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int l = loop_of[h];
    keys[h] = (unsigned)l < (unsigned)L && capped[l] ? l : -1;
}

__global__ __launch_bounds__(BLOCK) void cap_vertex_kernel(const float *__restrict__ verts, const unsigned char *__restrict__ colors,
                                                          const int *__restrict__ faces, int V, int L,
                                                          const int *__restrict__ capped, const int *__restrict__ loop_rank,
                                                          const int *__restrict__ loop_offsets, const int *__restrict__ loop_items,
                                                          int n_caps, float *__restrict__ new_verts,
                                                          unsigned char *__restrict__ new_colors) {
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= L || !capped[l]) return;
    const int o = loop_rank[l];
    const int lo = loop_offsets[l], hi = loop_offsets[l + 1];
    if (o >= n_caps || hi <= lo) return;                     // never: a capped loop has 3 .. max_edges half-edges
    double sx = 0.0, sy = 0.0, sz = 0.0;
    long long r = 0, g = 0, b = 0;
    for (int j = lo; j < hi; ++j) {
        const int a = faces[loop_items[j]];                  // the origin of the half-edge
        if ((unsigned)a >= (unsigned)V) continue;            // never: a boundary half-edge belongs to a checked face
        sx += (double)verts[3 * a];
        sy += (double)verts[3 * a + 1];
        sz += (double)verts[3 * a + 2];
        if (colors) {
            r += colors[3 * a];
            g += colors[3 * a + 1];
            b += colors[3 * a + 2];
        }
    }
    const double nd = (double)(hi - lo);
    new_verts[3 * o] = (float)(sx / nd);
    new_verts[3 * o + 1] = (float)(sy / nd);
    new_verts[3 * o + 2] = (float)(sz / nd);
    if (colors) {
        const long long n = hi - lo;
        new_colors[3 * o] = (unsigned char)((2 * r + n) / (2 * n));
        new_colors[3 * o + 1] = (unsigned char)((2 * g + n) / (2 * n));
        new_colors[3 * o + 2] = (unsigned char)((2 * b + n) / (2 * n));
    }
}

__global__ __launch_bounds__(BLOCK) void cap_face_kernel(const int *__restrict__ faces, int n, int V, int L,
                                                        const int *__restrict__ keys, const int *__restrict__ loop_rank,
                                                        const int *__restrict__ he_rank, int n_cap_faces,
                                                        int *__restrict__ new_faces) {
    const int h = blockIdx.x * BLOCK + threadIdx.x;
    if (h >= n) return;
    const int l = keys[h];
    if ((unsigned)l >= (unsigned)L) return;
    const int o = he_rank[h];
    if (o >= n_cap_faces) return;
    new_faces[3 * o] = faces[head_of(h)];                    // reversed: (b, a, centre)
    new_faces[3 * o + 1] = faces[h];
    new_faces[3 * o + 2] = V + loop_rank[l];
}

static inline bool count_ok(int64_t n) { return n >= 0 && n <= INT_MAX64; }
static inline bool faces_ok(int64_t F) { return F >= 0 && 3 * F <= INT_MAX64; }

// compress, flag the roots, rank them: total[0] = their number
static void rank_roots(int *parent, int n, int *is_root, int *wg, int *rank, int64_t *total, hipStream_t s) {
    hipLaunchKernelGGL(compress_kernel, dim3(blocks_for(n, BLOCK)), dim3(BLOCK), 0, s, parent, n, is_root);
    ranks<Flag, 1>(Flag{is_root}, n, wg, total, rank, s);
}

}  // namespace meshtopo
}  // namespace mvip

using namespace mvip;
namespace mt = mvip::meshtopo;

#define MT_GRID(n) dim3(blocks_for((n), mt::BLOCK)), dim3(mt::BLOCK), 0, s

extern "C" int mvip_mesh_topology_keys(const int *faces, int64_t n_faces, int64_t n_verts, int *keys, int *flag, void *stream) {
    if (!mt::faces_ok(n_faces) || !mt::count_ok(n_verts) || !flag) return MVIP_EINVAL;
    if (n_faces > 0 && (!faces || !keys)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = (int)(3 * n_faces);
    hipLaunchKernelGGL(mt::fill_kernel, dim3(1), dim3(mt::BLOCK), 0, s, flag, 1, 0);
    if (n > 0) hipLaunchKernelGGL(mt::keys_kernel, MT_GRID(n), faces, n, (int)n_verts, keys, flag);
    return check_launch();
}

extern "C" int mvip_mesh_topology_edges_find(const int *faces, int64_t n_faces, int64_t n_verts, const int *keys, const int *offsets,
                                             const int *items, int *rep, int *hcount, int *hforward, int *twin, int *wg, int *rank,
                                             int64_t *total, void *stream) {
    if (!mt::faces_ok(n_faces) || !mt::count_ok(n_verts) || n_verts + 1 > mt::INT_MAX64) return MVIP_EINVAL;
    if (n_faces == 0) return MVIP_OK;
    if (!faces || !keys || !offsets || !items || !rep || !hcount || !hforward || !twin || !wg || !rank || !total) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = (int)(3 * n_faces);
    hipLaunchKernelGGL(mt::edge_find_kernel, MT_GRID(n), faces, n, keys, offsets, items, rep, hcount, hforward, twin);
    mt::ranks<mt::IsOwn, 1>(mt::IsOwn{rep}, n, wg, total, rank, s);
    return check_launch();
}

extern "C" int mvip_mesh_topology_edges_emit(const int *faces, int64_t n_faces, const int *rep, const int *hcount,
                                             const int *hforward, const int *rank, int64_t n_edges, int *edge_of, int *edges,
                                             int *first, int *count, int *forward, void *stream) {
    if (!mt::faces_ok(n_faces) || n_edges < 0 || n_edges > 3 * n_faces) return MVIP_EINVAL;
    if (n_faces == 0) return MVIP_OK;
    if (!faces || !rep || !hcount || !hforward || !rank || !edge_of) return MVIP_EINVAL;
    if (n_edges > 0 && (!edges || !first || !count || !forward)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = (int)(3 * n_faces);
    hipLaunchKernelGGL(mt::edge_emit_kernel, MT_GRID(n), faces, n, rep, hcount, hforward, rank, (int)n_edges, edge_of, edges, first,
                       count, forward);
    return check_launch();
}

extern "C" int mvip_mesh_topology_components_label(const int *faces, int64_t n_faces, int64_t n_verts, int connectivity,
                                                   const int *rep, const int *offsets, const int *corners, int *parent,
                                                   int *is_root, int *wg, int *rank, int64_t *total, void *stream) {
    if (!mt::faces_ok(n_faces) || !mt::count_ok(n_verts) || (connectivity != 0 && connectivity != 1)) return MVIP_EINVAL;
    if (n_faces == 0) return MVIP_OK;
    if (!faces || !rep || !parent || !is_root || !wg || !rank || !total) return MVIP_EINVAL;
    if (connectivity == 1 && (!offsets || !corners)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int F = (int)n_faces, n = 3 * F;
    hipLaunchKernelGGL(mt::face_init_kernel, MT_GRID(F), rep, F, parent);
    if (connectivity == 0)
        hipLaunchKernelGGL(mt::face_union_edge_kernel, MT_GRID(n), rep, n, parent);
    else
        hipLaunchKernelGGL(mt::face_union_vertex_kernel, MT_GRID(n), faces, n, (int)n_verts, rep, offsets, corners, parent);
    mt::rank_roots(parent, F, is_root, wg, rank, total, s);
    return check_launch();
}

extern "C" int mvip_mesh_topology_components_emit(const int *faces, int64_t n_faces, int64_t n_verts, const int *parent,
                                                  const int *rank, int64_t n_components, const int *rep, const int *hcount,
                                                  const int *hforward, const int *offsets, const int *corners, int *labels,
                                                  int *table, void *stream) {
    if (!mt::faces_ok(n_faces) || !mt::count_ok(n_verts) || n_components < 0 || n_components > n_faces) return MVIP_EINVAL;
    if (n_faces == 0) return MVIP_OK;
    if (!faces || !parent || !rank || !rep || !hcount || !hforward || !offsets || !corners || !labels) return MVIP_EINVAL;
    if (n_components > 0 && !table) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int F = (int)n_faces, n = 3 * F, C = (int)n_components;
    if (C > 0) hipLaunchKernelGGL(mt::fill_kernel, MT_GRID(6 * (int64_t)C), table, 6 * C, 0);
    hipLaunchKernelGGL(mt::face_label_kernel, MT_GRID(F), parent, F, rank, C, labels, table);
    if (C > 0) {
        hipLaunchKernelGGL(mt::vertex_count_kernel, MT_GRID(n), faces, n, (int)n_verts, offsets, corners, (const int *)labels, C,
                           table);
        hipLaunchKernelGGL(mt::edge_count_kernel, MT_GRID(n), n, rep, hcount, hforward, (const int *)labels, C, table);
    }
    return check_launch();
}

extern "C" int mvip_mesh_topology_loops_label(const int *faces, int64_t n_faces, int64_t n_verts, const int *rep, const int *hcount,
                                              const int *offsets, const int *corners, int *ends, int *next, int *parent,
                                              int *is_root, int *wg, int *rank, int64_t *total, void *stream) {
    if (!mt::faces_ok(n_faces) || !mt::count_ok(n_verts)) return MVIP_EINVAL;
    if (n_faces == 0) return MVIP_OK;
    if (n_verts == 0 || !faces || !rep || !hcount || !offsets || !corners || !ends || !next || !parent || !is_root || !wg || !rank ||
        !total)
        return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = (int)(3 * n_faces), V = (int)n_verts;
    hipLaunchKernelGGL(mt::fill_kernel, MT_GRID(V), ends, V, 0);
    hipLaunchKernelGGL(mt::loop_ends_kernel, MT_GRID(n), faces, n, V, rep, hcount, ends);
    hipLaunchKernelGGL(mt::loop_next_kernel, MT_GRID(n), faces, n, V, rep, hcount, offsets, corners, (const int *)ends, next, parent);
    hipLaunchKernelGGL(mt::loop_union_kernel, MT_GRID(n), (const int *)next, n, parent);
    mt::rank_roots(parent, n, is_root, wg, rank, total, s);
    return check_launch();
}

extern "C" int mvip_mesh_topology_loops_emit(int64_t n_faces, const int *parent, const int *rank, const int *next, int64_t n_loops,
                                             int *loop_of, int *first, int *sizes, int *closed, void *stream) {
    if (!mt::faces_ok(n_faces) || n_loops < 0 || n_loops > 3 * n_faces) return MVIP_EINVAL;
    if (n_faces == 0) return MVIP_OK;
    if (!parent || !rank || !next || !loop_of) return MVIP_EINVAL;
    if (n_loops > 0 && (!first || !sizes || !closed)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = (int)(3 * n_faces), L = (int)n_loops;
    if (L > 0) {
        hipLaunchKernelGGL(mt::fill_kernel, MT_GRID(L), sizes, L, 0);
        hipLaunchKernelGGL(mt::fill_kernel, MT_GRID(L), closed, L, 1);
    }
    hipLaunchKernelGGL(mt::loop_emit_kernel, MT_GRID(n), parent, n, rank, next, L, loop_of, first, sizes, closed);
    return check_launch();
}

extern "C" int mvip_mesh_topology_cap_plan(int64_t n_faces, const int *loop_of, int64_t n_loops, const int *sizes, const int *closed,
                                           int64_t max_edges, int *capped, int *keys, int *loop_wg, int *loop_rank, int *he_wg,
                                           int *he_rank, int64_t *totals, void *stream) {
    if (!mt::faces_ok(n_faces) || n_loops < 0 || n_loops > 3 * n_faces || max_edges < 3) return MVIP_EINVAL;
    if (n_faces == 0) return MVIP_OK;
    if (!loop_of || !keys || !loop_wg || !he_wg || !he_rank || !totals) return MVIP_EINVAL;
    if (n_loops > 0 && (!sizes || !closed || !capped || !loop_rank)) return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = (int)(3 * n_faces), L = (int)n_loops;
    const int me = (int)(max_edges > mt::INT_MAX64 ? mt::INT_MAX64 : max_edges);
    if (L > 0) hipLaunchKernelGGL(mt::cap_choose_kernel, MT_GRID(L), sizes, closed, L, me, capped);
    hipLaunchKernelGGL(mt::cap_keys_kernel, MT_GRID(n), loop_of, n, L, (const int *)capped, keys);
    mt::ranks<mt::Flag, 1>(mt::Flag{capped}, L, loop_wg, totals, loop_rank, s);
    mt::ranks<mt::NonNegative, 1>(mt::NonNegative{keys}, n, he_wg, totals + 1, he_rank, s);
    return check_launch();
}

extern "C" int mvip_mesh_topology_cap_emit(const float *verts, const void *colors, const int *faces, int64_t n_verts,
                                           int64_t n_faces, int64_t n_loops, const int *keys, const int *capped,
                                           const int *loop_rank, const int *he_rank, const int *loop_offsets, const int *loop_items,
                                           int64_t n_caps, int64_t n_cap_faces, float *new_verts, void *new_colors, int *new_faces,
                                           void *stream) {
    if (!mt::faces_ok(n_faces) || !mt::count_ok(n_verts) || n_loops < 0 || n_loops > 3 * n_faces || n_caps < 0 ||
        n_caps > n_loops || n_cap_faces < 0 || n_cap_faces > 3 * n_faces || n_verts + n_caps > mt::INT_MAX64)
        return MVIP_EINVAL;
    if (n_caps == 0 || n_cap_faces == 0) return MVIP_OK;
    if (!verts || !faces || !keys || !capped || !loop_rank || !he_rank || !loop_offsets || !loop_items || !new_verts || !new_faces ||
        (colors && !new_colors))
        return MVIP_EINVAL;
    hipStream_t s = as_stream(stream);
    const int n = (int)(3 * n_faces), L = (int)n_loops, V = (int)n_verts;
    hipLaunchKernelGGL(mt::cap_vertex_kernel, MT_GRID(L), verts, (const unsigned char *)colors, faces, V, L, capped, loop_rank,
                       loop_offsets, loop_items, (int)n_caps, new_verts, (unsigned char *)new_colors);
    hipLaunchKernelGGL(mt::cap_face_kernel, MT_GRID(n), faces, n, V, L, keys, loop_rank, he_rank, (int)n_cap_faces, new_faces);
    return check_launch();
}
