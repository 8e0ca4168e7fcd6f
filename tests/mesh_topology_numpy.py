"""numpy restatement of the mesh topology (csrc/mesh_topology.hip; ops.mesh_edge_table / mesh_components /
mesh_boundary_loops / mesh_cap_loops), written from the definitions alone, by brute force: np.unique and a plain Python
union-find -- the role tests/mesh_ops_numpy.py has for the clean-up.

faces [F, 3] integers in [0, V).  Half-edge h = 3 f + k runs from a = faces[f, k] to b = faces[f, (k + 1) % 3].  A face that
names a vertex twice is degenerate and takes no part: edge_of = twin = -1, label 0, never a boundary.

Edge table: two half-edges of non-degenerate faces are one edge iff their unordered endpoints (lo, hi) are equal.  Edges are
numbered by ascending lowest half-edge `first`; count = half-edges of the edge, forward = those running lo -> hi; twin = the
other half-edge where count == 2, else -1.  boundary: count 1; interior: count 2, forward 1; inconsistent: count 2, forward
!= 1; non-manifold: count >= 3.

Components: 'edge' joins the faces of one edge, 'vertex' the non-degenerate faces of one vertex.  Labels 1..C by ascending
lowest face, 0 for degenerate faces.  table [C, 6]: faces, vertices (the distinct vertices of the component's faces), edges (by
the label of the face of the edge's first half-edge), and of those the boundary, non-manifold and inconsistent ones.

Loops: for a boundary half-edge h: a -> b, next[h] = the boundary half-edge starting at b if exactly one boundary half-edge
starts at b and exactly one ends there, else -1.  Loops = the components of h ~ next[h], numbered by ascending lowest
half-edge; closed iff every member has a next.

Caps: a loop is capped iff closed and 3 <= size <= max_edges.  New vertex = (fp64 sum of the fp32 origins of the loop's
half-edges in ascending half-edge order) / n, rounded once to fp32; colour (2 sum + n) // (2 n); numbered V, V + 1, ... in
loop order.  New face (b, a, new vertex) per half-edge of a capped loop, in ascending half-edge order.
"""
import collections

import numpy as np

EdgeTable = collections.namedtuple('EdgeTable', 'edge_of edges first count forward twin')
Loops = collections.namedtuple('Loops', 'loop_of next first sizes closed')
I32 = np.int32


def _faces(faces, n_verts):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= n_verts):
        raise ValueError('a face index lies outside [0, V)')
    return f


def degenerate(f):
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])


def half_edges(f):
    """origins a [3F], destinations b [3F], valid [3F] (the half-edges of non-degenerate faces)."""
    return f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1), np.repeat(~degenerate(f), 3)


class UnionFind:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        while self.p[x] != x:
            self.p[x] = self.p[self.p[x]]
            x = self.p[x]
        return x

    def unite(self, x, y):
        x, y = self.find(x), self.find(y)
        if x != y:
            self.p[max(x, y)] = min(x, y)


def edge_table(faces, n_verts):
    f = _faces(faces, n_verts)
    a, b, valid = half_edges(f)
    n = a.size
    edge_of, twin = np.full(n, -1, I32), np.full(n, -1, I32)
    hv = np.nonzero(valid)[0]
    if hv.size == 0:
        z = np.zeros(0, I32)
        return EdgeTable(edge_of, np.zeros((0, 2), I32), z, z, z, twin)
    lo, hi = np.minimum(a, b)[hv], np.maximum(a, b)[hv]
    _, first_at, inverse, count = np.unique(lo * n_verts + hi, return_index=True, return_inverse=True, return_counts=True)
    first = hv[first_at]                                       # np.unique returns the first occurrence: the lowest half-edge
    order = np.argsort(first)
    number = np.empty(order.size, np.int64)
    number[order] = np.arange(order.size)
    e = number[inverse.reshape(-1)]
    edge_of[hv] = e
    E = order.size
    forward = np.bincount(e, weights=(a[hv] == lo), minlength=E).astype(I32)
    edges = np.zeros((E, 2), I32)
    edges[e, 0], edges[e, 1] = lo, hi
    cnt = count[order].astype(I32)
    for k in np.nonzero(cnt == 2)[0]:
        h0, h1 = hv[e == k]
        twin[h0], twin[h1] = h1, h0
    return EdgeTable(edge_of, edges, first[order].astype(I32), cnt, forward, twin)


def components(faces, n_verts, connectivity='edge'):
    assert connectivity in ('edge', 'vertex')
    f = _faces(faces, n_verts)
    F = len(f)
    ok = ~degenerate(f) if F else np.zeros(0, bool)
    et = edge_table(f, n_verts)
    uf = UnionFind(F)
    groups = collections.defaultdict(list)
    if connectivity == 'edge':
        for h, e in enumerate(et.edge_of):
            if e >= 0:
                groups[int(e)].append(h // 3)
    else:
        for i in np.nonzero(ok)[0]:
            for v in f[i]:
                groups[int(v)].append(int(i))
    for members in groups.values():
        for m in members[1:]:
            uf.unite(members[0], m)
    roots = np.array([uf.find(i) if ok[i] else -1 for i in range(F)], np.int64)
    lowest = np.unique(roots[roots >= 0])                      # a root is the lowest face of its component
    labels = np.zeros(F, I32)
    labels[ok] = np.searchsorted(lowest, roots[ok]) + 1
    C = len(lowest)
    table = np.zeros((C, 6), I32)
    elab = labels[et.first // 3] if len(et.first) else np.zeros(0, I32)
    for c in range(1, C + 1):
        mine = elab == c
        table[c - 1] = (np.sum(labels == c), len(np.unique(f[labels == c])), np.sum(mine), np.sum(mine & (et.count == 1)),
                        np.sum(mine & (et.count >= 3)), np.sum(mine & (et.count == 2) & (et.forward != 1)))
    return labels, table


def boundary_loops(faces, n_verts):
    f = _faces(faces, n_verts)
    a, b, _ = half_edges(f)
    n = a.size
    et = edge_table(f, n_verts)
    on = np.zeros(n, bool)
    if n:
        on[et.edge_of >= 0] = et.count[et.edge_of[et.edge_of >= 0]] == 1
    bh = np.nonzero(on)[0]
    starts, ends = collections.defaultdict(list), collections.Counter()
    for h in bh:
        starts[int(a[h])].append(int(h))
        ends[int(b[h])] += 1
    nxt = np.full(n, -1, I32)
    for h in bh:
        v = int(b[h])
        if len(starts[v]) == 1 and ends[v] == 1:
            nxt[h] = starts[v][0]
    uf = UnionFind(n)
    for h in bh:
        if nxt[h] >= 0:
            uf.unite(int(h), int(nxt[h]))
    roots = np.array([uf.find(int(h)) for h in bh], np.int64)
    first = np.unique(roots)
    loop_of = np.full(n, -1, I32)
    loop_of[bh] = np.searchsorted(first, roots)
    L = len(first)
    sizes = np.bincount(loop_of[bh], minlength=L).astype(I32)
    closed = np.ones(L, I32)
    closed[loop_of[bh][nxt[bh] < 0]] = 0
    return Loops(loop_of, nxt, first.astype(I32), sizes, closed)


def cap_loops(verts, faces, colors, max_edges):
    """-> (new_verts fp32 [N, 3], new_colors uint8 [N, 3] | None, new_faces int32 [M, 3], capped int32 [L])."""
    v = np.asarray(verts, np.float32)
    V = len(v)
    f = _faces(faces, V)
    a, b, _ = half_edges(f)
    lp = boundary_loops(f, V)
    capped = ((lp.closed != 0) & (lp.sizes >= 3) & (lp.sizes <= max_edges)).astype(I32)
    number = np.cumsum(capped) - 1
    new_v, new_c = [], []
    for l in np.nonzero(capped)[0]:
        s = np.zeros(3, np.float64)
        for h in np.nonzero(lp.loop_of == l)[0]:               # ascending half-edges, one by one
            s = s + v[a[h]].astype(np.float64)
        n = int(lp.sizes[l])
        new_v.append((s / np.float64(n)).astype(np.float32))
        if colors is not None:
            tot = np.asarray(colors, np.uint8)[a[lp.loop_of == l]].astype(np.int64).sum(0)
            new_c.append(((2 * tot + n) // (2 * n)).astype(np.uint8))
    hs = np.nonzero((lp.loop_of >= 0) & (capped[np.maximum(lp.loop_of, 0)] != 0 if len(capped) else False))[0]
    new_f = np.stack([b[hs], a[hs], V + number[lp.loop_of[hs]]], -1).astype(I32).reshape(-1, 3)
    return (np.asarray(new_v, np.float32).reshape(-1, 3), None if colors is None else np.asarray(new_c, np.uint8).reshape(-1, 3),
            new_f, capped)


# ---- what mesh.topology reports, from the tables alone ----------------------------------------------------------------------
def report(faces, n_verts, connectivity='edge'):
    f = _faces(faces, n_verts)
    labels, table = components(f, n_verts, connectivity)
    lp = boundary_loops(f, n_verts)
    tot = table.sum(0) if len(table) else np.zeros(6, np.int64)
    closed = bool(tot[3] == 0 and tot[4] == 0)
    oriented = bool(tot[5] == 0 and tot[4] == 0)
    euler = int(tot[1] - tot[2] + tot[0])
    return dict(faces=int(tot[0]), vertices=int(tot[1]), edges=int(tot[2]), boundary_edges=int(tot[3]),
                non_manifold_edges=int(tot[4]), inconsistent_edges=int(tot[5]), components=len(table), closed=closed,
                oriented=oriented, euler=euler, genus=(2 * len(table) - euler) // 2 if closed and oriented else None,
                loops=len(lp.first), closed_loops=int(lp.closed.sum()))


# ---- meshes built for the kernels' weak points -------------------------------------------------------------------------------
def strip(n=4096, mult=2731):
    """A strip of n triangles between two rows of vertices (even vertices below, odd above), counter-clockwise, its faces
    permuted by i -> mult * i mod n: one component, one boundary loop of n + 2 half-edges."""
    V = n + 2
    t = np.arange(n, dtype=np.int64)
    tri = np.where((t % 2 == 0)[:, None], np.stack([t, t + 2, t + 1], -1), np.stack([t, t + 1, t + 2], -1))
    faces = np.empty_like(tri)
    faces[(mult * t) % n] = tri
    x = (np.arange(V) // 2).astype(np.float32) * np.float32(0.37)
    verts = np.stack([x, (np.arange(V) % 2).astype(np.float32), np.sin(x).astype(np.float32)], -1).astype(np.float32)
    return verts, faces.astype(I32)


def fan(n=300):
    """n triangles round vertex 0 (a closed disc sector ring: rim vertices 1..n, the last joined to the first)."""
    k = np.arange(n, dtype=np.int64)
    faces = np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], -1)
    ang = 2 * np.pi * k / n
    verts = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], -1)]).astype(np.float32)
    return verts, faces.astype(I32)


# ---- the meshes of the tests: marching cubes (tests/mc_numpy.py) of the lattices of tests/mesh_ops_numpy.py, iso value 1 --------
_cache = {}


def mc_mesh(case):
    """(verts fp32 [V, 3], faces int64 [F, 3]) of CLUSTER_CASES entry `case` ('sphere24_3', 'two_spheres24_2.5', 'torus32_6')."""
    import mc_numpy as M
    import mesh_ops_numpy as R
    if case not in _cache:
        _, npts, fn, _, _ = next(c for c in R.CLUSTER_CASES if c[0] == case)
        v, f, _ = M.marching_cubes(R.lattice(npts, fn), 1.0, R.LO, R.HI)
        v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64)
        v.setflags(write=False)
        f.setflags(write=False)
        _cache[case] = (v, f)
    return _cache[case]


def cut(v, f, axis, bound, absolute=False):
    """the faces whose three vertices all have coordinate `axis` (or its magnitude) below `bound`; the vertices stay."""
    x = v[f][:, :, axis]
    return f[np.all((np.abs(x) if absolute else x) < bound, axis=1)]
