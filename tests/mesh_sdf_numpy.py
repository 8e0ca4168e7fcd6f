"""numpy restatement of the signed mesh distance (csrc/mesh_sdf.hip; ops.mesh_vertex_pseudonormals / mesh_signed_distance /
mesh_signed_distance_lattice), written from the definitions alone.  BRUTE FORCE: every query against every face, no grid.

All arithmetic is fp64 on the widened fp32 inputs; a dot product is (x0 y0 + x1 y1) + x2 y2; results are rounded to fp32 once.

Closest feature: face(p), q and d2 are those of tests/mesh_distance_numpy.py (interior, then the segments ab, bc, ca, a later
candidate replacing an earlier one only where strictly smaller; the lowest face among equals).  The candidate of the winning
face that supplied q: 0 the interior; segment k with 0 < t < 1: 1 + k; with t == 0 (ee == 0 included): 4 + k; with t == 1:
4 + (k + 1) % 3.

Pseudonormal n.  N(f) = (b - a) x (c - a); U(f) = N / sqrt(N . N), zeros if N . N == 0.
  interior: N(f).  edge h = 3 f + k: U(f) + U(twin[h] // 3) if twin[h] >= 0 else U(f), twin that of the edge table (exactly two
  half-edges on the edge).  vertex v: P[v] = the sum over v's corners c = 3 f + k, ascending, of theta_c U(f),
  theta_c = atan2(sqrt(X . X), u . w), X = u x w, u = faces[f, (k + 1) % 3] - v, w = faces[f, (k + 2) % 3] - v.

Sign: s = n . (p - q), q unrounded; sdist = fp32(sqrt(d2)), negated iff s < 0 and d2 > 0.
Band B: out of band iff d2 > B B: face -1, feature -1, sdist and point NaN, as for a query with a NaN or infinite coordinate.
Lattice: point (i, j, k), k fastest, = fp32(fp32(i) h) + lo per axis in fp32.
"""
import numpy as np

import mesh_distance_numpy as D
import mesh_topology_numpy as T

F32, F64 = np.float32, np.float64


def _segment(k, p, u, e, d2, q, feat):
    ee = D._dot3(e, e)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = D._dot3(D._sub3(p, u), e) / ee
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    t = np.where(ee > 0.0, t, 0.0)
    s = (u[0] + t * e[0], u[1] + t * e[1], u[2] + t * e[2])
    d = D._sub3(p, s)
    s2 = D._dot3(d, d)
    nearer = s2 < d2
    code = np.where(t == 0.0, 4 + k, np.where(t == 1.0, 4 + (k + 1) % 3, 1 + k))
    return np.where(nearer, s2, d2), tuple(np.where(nearer, s[i], q[i]) for i in range(3)), np.where(nearer, code, feat)


def _point_triangle(p, a, b, c):
    """(d2, q triple, feature) for triples of arrays of any shapes that broadcast"""
    ab, ac, bc, ca = D._sub3(b, a), D._sub3(c, a), D._sub3(c, b), D._sub3(a, c)
    N = D._cross3(ab, ac)
    nn = D._dot3(N, N)
    ap = D._sub3(p, a)
    e0 = D._dot3(N, D._cross3(ab, ap))
    e1 = D._dot3(N, D._cross3(bc, D._sub3(p, b)))
    e2 = D._dot3(N, D._cross3(ca, D._sub3(p, c)))
    inside = (nn > 0.0) & (e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)
    s = D._dot3(N, ap)
    with np.errstate(divide='ignore', invalid='ignore'):
        k = s / nn
        d2 = np.where(inside, s * s / nn, np.inf)
        q = tuple(np.where(inside, p[t] - N[t] * k, a[t]) for t in range(3))
    feat = np.where(inside, 0, 4)
    d2, q, feat = _segment(0, p, a, ab, d2, q, feat)
    d2, q, feat = _segment(1, p, b, bc, d2, q, feat)
    d2, q, feat = _segment(2, p, c, ca, d2, q, feat)
    return d2, q, feat


def point_triangle(points, a, b, c):
    """(d2 [N, F] fp64, q [N, F, 3] fp64, feature [N, F]) for points [N, 3] and the faces' vertices a, b, c [F, 3]"""
    pts = np.asarray(points, F64)
    p = tuple(pts[:, k, None] for k in range(3))
    a, b, c = (tuple(np.asarray(x, F64)[None, :, k] for k in range(3)) for x in (a, b, c))
    d2, q, feat = _point_triangle(p, a, b, c)
    return d2, np.stack(q, -1), feat


def _candidates(pts, a, b, c):
    """(query index [M], face index [M]), sorted by query then face: every pair that can hold the smallest d2 of its query or tie
    with it.  A face is left out only where the distance to its bounding box exceeds, by more than a factor 1 + 1e-9, the
    distance to some face's first vertex -- an upper bound on the smallest d2.  What is evaluated on the pairs is the same
    arithmetic: leaving out a face that cannot win changes no output."""
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    d = pts[:, None, :] - a[None]
    ub = D._dot(d, d).min(axis=1)
    gap = np.maximum(np.maximum(lo[None] - pts[:, None, :], pts[:, None, :] - hi[None]), 0.0)
    keep = D._dot(gap, gap) <= ub[:, None] * (1.0 + 1e-9) + 1e-300
    return np.nonzero(keep)


def closest_feature(points, verts, faces, chunk=1 << 18, prune=False):
    """(face [N] int32, q [N, 3] fp64 unrounded, d2 [N] fp64, feature [N] int32) by brute force over the finite queries; the
    others: face -1, q and d2 NaN, feature -1.  prune=True: only the pairs of _candidates() are evaluated (the same result,
    tests/test_mesh_sdf_cpu.py; for the meshes of a few thousand faces)."""
    pts = np.asarray(points, F32)
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v) and np.all(np.isfinite(v))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = len(pts)
    face, feat = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    q, best = np.full((n, 3), np.nan, F64), np.full(n, np.nan, F64)
    ok = np.nonzero(np.all(np.isfinite(pts), axis=1))[0]
    rows = max(1, chunk // len(f))
    for s in range(0, len(ok), rows):
        idx = ok[s:s + rows]
        if prune:
            pp = pts[idx].astype(F64)
            qi, fi = _candidates(pp, a, b, c)
            d2, qq, ft = _point_triangle(tuple(pp[qi, t] for t in range(3)), tuple(a[fi, t] for t in range(3)),
                                         tuple(b[fi, t] for t in range(3)), tuple(c[fi, t] for t in range(3)))
            start = np.searchsorted(qi, np.arange(len(idx)))                        # every query has a candidate
            low = np.minimum.reduceat(d2, start)
            first = np.nonzero(d2 == low[qi])[0]                                   # ascending: the lowest face of a query first
            first = first[np.unique(qi[first], return_index=True)[1]]
            face[idx], best[idx], feat[idx] = fi[first], d2[first], ft[first]
            q[idx] = np.stack([qq[t][first] for t in range(3)], -1)
            continue
        d2, qq, ft = point_triangle(pts[idx].astype(F64), a, b, c)
        k = np.argmin(d2, axis=1)                                                  # the first (lowest face) among equal minima
        r = np.arange(len(idx))
        face[idx], q[idx], best[idx], feat[idx] = k, qq[r, k], d2[r, k], ft[r, k]
    return face, q, best, feat


def face_normals(verts, faces):
    """(N [F, 3], U [F, 3]) fp64"""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    N = D._cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    nn = D._dot(N, N)
    with np.errstate(divide='ignore', invalid='ignore'):
        U = np.where((nn > 0.0)[:, None], N / np.sqrt(nn)[:, None], 0.0)
    return N, U


def corner_angles(verts, faces):
    """theta [F, 3] fp64"""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros((len(f), 3), F64)
    for k in range(3):
        o = v[f[:, k]]
        u, w = v[f[:, (k + 1) % 3]] - o, v[f[:, (k + 2) % 3]] - o
        X = D._cross(u, w)
        out[:, k] = np.arctan2(np.sqrt(D._dot(X, X)), D._dot(u, w))
    return out


def vertex_pseudonormals(verts, faces, weighted=True):
    """P [V, 3] fp64: per vertex the sum over its corners, ascending, of theta_c U(f) (weighted=False: of U(f) alone -- NOT the
    definition, the comparison of the CPU tests)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    _, U = face_normals(verts, f)
    theta = corner_angles(verts, f) if weighted else np.ones((len(f), 3), F64)
    P = np.zeros((len(np.asarray(verts).reshape(-1, 3)), 3), F64)
    for fi in range(len(f)):                                                       # corners ascending: face-major, then k
        for k in range(3):
            vtx = f[fi, k]
            for t in range(3):
                P[vtx, t] = P[vtx, t] + theta[fi, k] * U[fi, t]
    return P


def n_corners(faces, n_verts):
    return np.bincount(np.asarray(faces, np.int64).reshape(-1), minlength=n_verts)


def twins(faces, n_verts):
    return np.asarray(T.edge_table(np.asarray(faces, np.int32).reshape(-1, 3), n_verts).twin, np.int64)


def pseudonormal_of(face, feat, verts, faces, P, twin, mode='pseudonormal'):
    """n [N, 3] fp64 for the winning face and feature of each query (rows with face -1: zeros).  mode 'face': N(f) whatever the
    feature -- NOT the definition, the comparison of the CPU tests."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    N, U = face_normals(verts, f)
    face, feat = np.asarray(face, np.int64), np.asarray(feat, np.int64)
    ok = face >= 0
    fa = np.where(ok, face, 0)
    n = np.where(ok[:, None], N[fa], 0.0)
    if mode == 'face':
        return n
    edge = ok & (feat >= 1) & (feat <= 3)
    h = 3 * fa + np.where(edge, feat - 1, 0)
    tw = np.asarray(twin, np.int64)[h]
    both = U[fa] + U[np.where(tw >= 0, tw, 0) // 3]
    n = np.where(edge[:, None], np.where((tw >= 0)[:, None], both, U[fa]), n)
    vert = ok & (feat >= 4)
    vtx = f[fa, np.where(vert, feat - 4, 0)]
    return np.where(vert[:, None], np.asarray(P, F64)[vtx], n)


def signed_distance(points, verts, faces, P=None, twin=None, max_dist=None, mode='pseudonormal', closest=None, chunk=1 << 18,
                    prune=False):
    """(sdist [N] fp32, face [N] int32, point [N, 3] fp32, feature [N] int32, d2 [N] fp64).  P / twin None: this file's own.
    closest: a closest_feature() result of these queries to reuse."""
    pts = np.asarray(points, F32)
    nv = len(np.asarray(verts).reshape(-1, 3))
    P = vertex_pseudonormals(verts, faces) if P is None else P
    twin = twins(faces, nv) if twin is None else twin
    face, q, d2, feat = closest_feature(pts, verts, faces, chunk, prune) if closest is None else closest
    if max_dist is not None:
        B = float(max_dist)
        with np.errstate(invalid='ignore'):
            out = d2 > B * B
        face, feat = np.where(out, -1, face).astype(np.int32), np.where(out, -1, feat).astype(np.int32)
        q, d2 = np.where(out[:, None], np.nan, q), np.where(out, np.nan, d2)
    n = pseudonormal_of(face, feat, verts, faces, P, twin, mode)
    ok = face >= 0
    d = pts.astype(F64) - np.where(ok[:, None], q, 0.0)
    s = D._dot(n, np.where(ok[:, None], d, 0.0))
    with np.errstate(invalid='ignore'):
        dist = np.sqrt(d2).astype(F32)
        sd = np.where(ok & (s < 0.0) & (d2 > 0.0), -dist, dist).astype(F32)
    return sd, face.astype(np.int32), q.astype(F32), feat.astype(np.int32), d2


def lattice_points(lo, h, counts):
    """[nx ny nz, 3] fp32, k fastest: fp32(fp32(i) h) + lo"""
    axes = [(np.arange(counts[a], dtype=F32) * F32(h[a]) + F32(lo[a])).astype(F32) for a in range(3)]
    g = np.meshgrid(*axes, indexing='ij')
    return np.stack([x.reshape(-1) for x in g], -1).astype(F32)


# ---- the small closed meshes of the tests, with their analytic inside test ----------------------------------------------------
def tetrahedron():
    """the regular tetrahedron on alternate corners of the cube +-0.5, outward faces"""
    v = np.asarray([[0.5, 0.5, 0.5], [0.5, -0.5, -0.5], [-0.5, 0.5, -0.5], [-0.5, -0.5, 0.5]], F32)
    f = np.asarray([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)
    return v, orient_outward(v, f)


def orient_outward(v, f):
    """each face of a convex mesh turned so that its normal points away from the centroid of the vertices"""
    f = np.asarray(f, np.int32).copy()
    c = np.asarray(v, F64).mean(0)
    N, _ = face_normals(v, f)
    flip = D._dot(N, np.asarray(v, F64)[f[:, 0]] - c) < 0
    f[flip] = f[flip][:, ::-1]
    return f


SPIKE_R = 0.1


def _spike_base():
    ang = np.deg2rad([90.0, 210.0, 330.0])
    return np.stack([SPIKE_R * np.cos(ang), SPIKE_R * np.sin(ang), np.zeros(3)], -1)


def spike():
    """apex (0, 0, 1) over a triangle of radius 0.1 in z = 0: 4 faces"""
    v = np.concatenate([[[0.0, 0.0, 1.0]], _spike_base()]).astype(F32)
    f = np.asarray([(0, 1, 2), (0, 2, 3), (0, 3, 1), (1, 3, 2)], np.int32)
    return v, orient_outward(v, f)


def fan_spike(n=16):
    """the spike with the side face over base edge 1-2 split into n slivers at the apex, the base re-fanned from vertex 3 so that
    the mesh stays closed: 2 + n + n = 34 faces for n = 16"""
    base = _spike_base()
    t = (np.arange(1, n, dtype=F64) / n)[:, None]
    mid = base[0] * (1.0 - t) + base[1] * t                                        # n - 1 new vertices on base edge 1-2
    v = np.concatenate([[[0.0, 0.0, 1.0]], base, mid]).astype(F32)
    chain = [1] + list(range(4, 4 + n - 1)) + [2]
    f = [(0, chain[i], chain[i + 1]) for i in range(n)] + [(0, 2, 3), (0, 3, 1)] + [(3, chain[i + 1], chain[i]) for i in range(n)]
    return v, orient_outward(v, np.asarray(f, np.int32))


def convex_inside(points, verts, faces):
    """(inside [N] bool, margin [N] fp64): the half-space test of a convex mesh -- inside iff every face plane has the point
    behind it; margin = the smallest |plane distance|, to tell a point that sits on a plane."""
    _, U = face_normals(verts, faces)
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(points, F32).astype(F64)
    h = np.einsum('nfk,fk->nf', p[:, None, :] - v[f[:, 0]][None], U)
    return np.all(h < 0.0, axis=1), np.abs(h).min(axis=1)


def open_degenerate():
    """a unit square of two triangles (open: a boundary loop), a zero-area face on its diagonal, a point face, a free vertex"""
    v = np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 0], [0.25, 0.5, 0.75], [2, 2, 2]], F32)
    f = np.asarray([(0, 1, 2), (0, 2, 3), (0, 4, 2), (5, 5, 5)], np.int32)
    return v, f


def feature_queries(verts, faces):
    """[V + 3 F + F, 3] fp32: every vertex, every edge midpoint, every face centroid -- queries at (or within an fp32 rounding of)
    distance zero, on every kind of feature"""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    mids = [(v[f[:, k]] + v[f[:, (k + 1) % 3]]) / 2.0 for k in range(3)]
    cen = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / 3.0
    return np.concatenate([v] + mids + [cen]).astype(F32)


BAD_ROWS = np.asarray([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]], F32)


def query_set(verts, faces, n_random, seed, grow=0.5):
    """n_random seed-`seed` uniform points in the bounding box grown by `grow` of its largest extent, then feature_queries, then
    BAD_ROWS"""
    v = np.asarray(verts, F32).astype(F64)
    lo, hi = v.min(0), v.max(0)
    pad = grow * float((hi - lo).max())
    rnd = np.random.default_rng(seed).uniform(lo - pad, hi + pad, (n_random, 3)).astype(F32)
    return np.concatenate([rnd, feature_queries(verts, faces), BAD_ROWS]).astype(F32)
