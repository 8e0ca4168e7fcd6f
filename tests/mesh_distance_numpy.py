"""numpy restatement of the mesh-to-mesh distance (csrc/mesh_distance.hip; ops.mesh_closest_point / mesh_sample_faces,
evaluate.mesh_distance_metrics), written from the definitions alone -- the role tests/raster_numpy.py has for the rasteriser.
It is BRUTE FORCE: every query against every face, no grid; the kernel's result must not depend on its grid.

verts [V, 3] fp32, faces [F, 3] integers, points [N, 3] fp32.  All arithmetic is fp64 on the widened fp32 inputs; a dot product is
(x0 y0 + x1 y1) + x2 y2; results are rounded to fp32 once.

Point - triangle: squared distance d2 and closest point q of p to the face (a, b, c) = the first of four candidates, a later one
replacing an earlier one only where strictly smaller:
  interior: N = (b - a) x (c - a), nn = N . N; taken iff nn > 0 and N . ((b - a) x (p - a)) >= 0, N . ((c - b) x (p - b)) >= 0,
    N . ((a - c) x (p - c)) >= 0; s = N . (p - a), d2 = s s / nn, q = p - N (s / nn);
  segments ab, bc, ca (from u along e): ee = e . e, t = ((p - u) . e) / ee, 0 where t < 0, 1 where t > 1, 0 where ee == 0;
    q = u + t e, d2 = (p - q) . (p - q).
Closest point on a mesh: the face of smallest d2, the lowest index among equals; point = fp32(q), dist = fp32(sqrt(d2)); a query
with a NaN or infinite coordinate: face -1, point and dist NaN.

Samples, subdivision k: sample s of a face, s < k (k + 1) / 2: the upward triangle (i, j), i + j < k, i ascending then j,
(na, nb) = (3 i + 1, 3 j + 1); then the downward triangles (i, j), i + j < k - 1, same order, (na, nb) = (3 i + 2, 3 j + 2);
nc = 3 k - na - nb; point = fp32(((na a + nb b) + nc c) / (3 k)); weight = (sqrt(N . N) / 2) / k^2.  Face-major.

Report: see distance_report().
"""
import numpy as np

F32, F64 = np.float32, np.float64


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _dot3(x, y):
    """vectors as triples of arrays (x, y, z): no stacking, the same sums"""
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _cross3(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def _sub3(x, y):
    return (x[0] - y[0], x[1] - y[1], x[2] - y[2])


def _segment(p, u, e, d2, q):
    """candidates of the segment from u along e (triples of [1, F]) for p (triple of [N, 1]); replaces (d2 [N, F], q triple of
    [N, F]) where strictly nearer"""
    ee = _dot3(e, e)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = _dot3(_sub3(p, u), e) / ee
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    t = np.where(ee > 0.0, t, 0.0)
    s = (u[0] + t * e[0], u[1] + t * e[1], u[2] + t * e[2])
    d = _sub3(p, s)
    s2 = _dot3(d, d)
    nearer = s2 < d2
    return np.where(nearer, s2, d2), tuple(np.where(nearer, s[k], q[k]) for k in range(3))


def point_triangle(points, a, b, c):
    """(d2 [N, F] fp64, q [N, F, 3] fp64) for points [N, 3] and the faces' vertices a, b, c [F, 3] (fp64 values of fp32 numbers)."""
    pts = np.asarray(points, F64)
    p = tuple(pts[:, k, None] for k in range(3))                                   # [N, 1]
    a, b, c = (tuple(np.asarray(x, F64)[None, :, k] for k in range(3)) for x in (a, b, c))     # [1, F]
    ab, ac, bc, ca = _sub3(b, a), _sub3(c, a), _sub3(c, b), _sub3(a, c)
    N = _cross3(ab, ac)
    nn = _dot3(N, N)
    ap = _sub3(p, a)
    e0 = _dot3(N, _cross3(ab, ap))
    e1 = _dot3(N, _cross3(bc, _sub3(p, b)))
    e2 = _dot3(N, _cross3(ca, _sub3(p, c)))
    inside = (nn > 0.0) & (e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)
    s = _dot3(N, ap)
    with np.errstate(divide='ignore', invalid='ignore'):
        k = s / nn
        d2 = np.where(inside, s * s / nn, np.inf)
        q = tuple(np.where(inside, p[t] - N[t] * k, a[t]) for t in range(3))
    d2, q = _segment(p, a, ab, d2, q)
    d2, q = _segment(p, b, bc, d2, q)
    d2, q = _segment(p, c, ca, d2, q)
    return d2, np.stack(q, -1)


def closest_point(points, verts, faces, chunk=1 << 18):
    """(face [N] int32, point [N, 3] fp32, dist [N] fp32, d2 [N] fp64) by brute force, `chunk` point-face tests at a time."""
    pts = np.asarray(points, F32)
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v) and np.all(np.isfinite(v))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = len(pts)
    face = np.full(n, -1, np.int32)
    point = np.full((n, 3), np.nan, F32)
    dist = np.full(n, np.nan, F32)
    best = np.full(n, np.nan, F64)
    ok = np.nonzero(np.all(np.isfinite(pts), axis=1))[0]
    rows = max(1, chunk // len(f))
    for s in range(0, len(ok), rows):
        idx = ok[s:s + rows]
        d2, q = point_triangle(pts[idx].astype(F64), a, b, c)
        k = np.argmin(d2, axis=1)                                                  # the first (lowest face) among equal minima
        r = np.arange(len(idx))
        face[idx] = k
        point[idx] = q[r, k].astype(F32)
        best[idx] = d2[r, k]
        dist[idx] = np.sqrt(d2[r, k]).astype(F32)
    return face, point, dist, best


def sample_order(k):
    """[(na, nb, nc)] of the k^2 samples of a face, in order."""
    out = [(3 * i + 1, 3 * j + 1) for i in range(k) for j in range(k - i)]
    out += [(3 * i + 2, 3 * j + 2) for i in range(k - 1) for j in range(k - 1 - i)]
    assert len(out) == k * k
    return [(na, nb, 3 * k - na - nb) for na, nb in out]


def face_areas(verts, faces):
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    N = _cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return np.sqrt(_dot(N, N)) / 2.0


def sample_faces(verts, faces, k):
    """(points [F k^2, 3] fp32, face_of_sample [F k^2] int32, weights [F k^2] fp64)"""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.asarray(sample_order(k), F64)                                            # [k^2, 3]
    na, nb, nc = (n[None, :, t, None] for t in range(3))
    pts = ((na * a[:, None] + nb * b[:, None]) + nc * c[:, None]) / F64(3 * k)
    w = np.repeat(face_areas(verts, faces) / F64(k * k), k * k)
    return pts.reshape(-1, 3).astype(F32), np.repeat(np.arange(len(f), dtype=np.int32), k * k), w


def unit_normals(verts, faces):
    """(unit normals [F, 3] fp64, zero for a degenerate face; degenerate [F] bool): N / sqrt(N . N), degenerate iff not N . N > 0."""
    v = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    N = _cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    nn = _dot(N, N)
    bad = ~(nn > 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        u = np.where(bad[:, None], 0.0, N / np.sqrt(nn)[:, None])
    return u, bad


def direction_report(dist, weights, normals_from, face_of_sample, normals_to, hit_face, thresholds):
    """One direction of the report, from the distances of a mesh's samples to the other mesh.  Every sum is numpy's sum of the
    elementwise products in sample order, in fp64: W = sum(w); mean = sum(w d) / W; rms = sqrt(sum(w d d) / W); max = max(d);
    within[tau] = sum(w where d <= tau) / W; normal_consistency = sum(w |n . n'|) / sum(w) over the samples whose own face and
    hit face both are non-degenerate."""
    d = np.asarray(dist, F32).astype(F64)
    w = np.asarray(weights, F64)
    W = np.sum(w)
    nf, bad_f = normals_from
    nt, bad_t = normals_to
    fos, hit = np.asarray(face_of_sample, np.int64), np.asarray(hit_face, np.int64)
    ok = ~bad_f[fos] & ~bad_t[hit]
    c = np.abs(_dot(nf[fos], nt[hit]))
    wk = np.where(ok, w, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return {'samples': int(len(d)), 'area': float(W), 'mean': float(np.sum(w * d) / W), 'rms': float(np.sqrt(np.sum(w * d * d) / W)),
                'max': float(np.max(d)), 'within': [float(np.sum(np.where(d <= F64(t), w, 0.0)) / W) for t in thresholds],
                'normal_consistency': float(np.sum(wk * c) / np.sum(wk))}


def distance_report(ab, ba, thresholds):
    """The combined report from the two directions' direction_report()s: chamfer = (mean_ab + mean_ba) / 2, hausdorff = the larger
    maximum, precision = within of a -> b, recall = within of b -> a, fscore = 2 P R / (P + R) (0 where P + R == 0),
    normal_consistency = the mean of the two directions'."""
    P, R = ab['within'], ba['within']
    return {'thresholds': [float(t) for t in thresholds], 'a_to_b': ab, 'b_to_a': ba, 'chamfer': (ab['mean'] + ba['mean']) / 2.0,
            'hausdorff': max(ab['max'], ba['max']), 'precision': list(P), 'recall': list(R),
            'fscore': [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(P, R)],
            'normal_consistency': (ab['normal_consistency'] + ba['normal_consistency']) / 2.0}


def mesh_distance_metrics(va, fa, vb, fb, samples=2, thresholds=()):
    """The whole report by brute force (small meshes)."""
    out = []
    for (v0, f0), (v1, f1) in (((va, fa), (vb, fb)), ((vb, fb), (va, fa))):
        pts, fos, w = sample_faces(v0, f0, samples)
        face, _, dist, _ = closest_point(pts, v1, f1)
        out.append(direction_report(dist, w, unit_normals(v0, f0), fos, unit_normals(v1, f1), face, thresholds))
    return distance_report(out[0], out[1], thresholds)


# ---- the analytic meshes of the CPU tests ------------------------------------------------------------------------------------
def square_mesh(n, z, flip=False):
    """the unit square [0, 1]^2 in the plane `z`, n x n cells of two triangles each (coordinates k / n: exact for n a power of two)"""
    ax = np.arange(n + 1, dtype=F64) / n
    x, y = np.meshgrid(ax, ax, indexing='ij')
    v = np.stack([x.reshape(-1), y.reshape(-1), np.full((n + 1) ** 2, z)], -1).astype(F32)
    idx = lambda i, j: i * (n + 1) + j
    f = []
    for i in range(n):
        for j in range(n):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    f = np.asarray(f, np.int32)
    return v, (f[:, ::-1].copy() if flip else f)


def cube_mesh(half, centre=(0.0, 0.0, 0.0)):
    """the cube of half-edge `half` about `centre`: 8 vertices, 12 outward triangles"""
    s = np.asarray([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F64)
    v = (np.asarray(centre, F64) + half * s).astype(F32)
    f = np.asarray([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                    (1, 5, 7), (1, 7, 3)], np.int32)
    return v, f
