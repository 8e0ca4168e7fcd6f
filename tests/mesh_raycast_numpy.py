"""numpy restatement of mesh ray casting (csrc/mesh_raycast.hip; ops.mesh_cast_rays / mesh_occluded / mesh_face_openness),
written from the definitions alone -- the role tests/mesh_distance_numpy.py has for the closest point.  It is BRUTE FORCE: every
ray against every face, no grid; the kernel's result must not depend on its grid.

verts [V, 3] fp32, faces [F, 3] integers.  A ray is (o[3], d[3], tmin, tmax) in fp32 (the openness sweep passes its fp64
centroids as origins).  All arithmetic is fp64 on the widened inputs, every expression associates as written.

Ray - triangle (the watertight test of Woop, Benthin, Wald 2013): kz = the axis of largest |d|, the lowest among equals; kx, ky
the next two cyclically, swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  A vertex P becomes
A = P - o, Px = A[kx] - Sx A[kz], Py = A[ky] - Sy A[kz], Pz = Sz A[kz] -- the same numbers whichever face it belongs to.  With
(A, B, C) the transformed vertices of the face: U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax; a candidate iff all
three are >= 0 or all three are <= 0 (no culling); det = (U + V) + W must be non-zero; t = ((U Az + V Bz) + W Cz) / det; hit iff
tmin <= t <= tmax.

Result: the hit of smallest fp64 t, the lowest face index among equals, except the face skip[n] (-1: none); face int32 (-1: a
miss), t = fp32(t) (+inf: a miss), bary = (fp32(V / det), fp32(W / det)) (NaN without a hit).  An invalid ray -- a NaN or infinite
component of o or d, d = 0, tmin not finite, tmax NaN or < tmin (tmax = +inf is allowed) -- gives face -1, t NaN.
Occlusion is face >= 0.

Openness of face f for directions d_k [K, 3] fp32: origin = the fp64 centroid ((a + b) + c) / 3, N = (b - a) x (c - a);
d_k is on the front side iff N . d_k > 0, on the back side iff < 0, skipped iff == 0 (N . d = (N0 d0 + N1 d1) + N2 d2); open iff
the ray (centroid, d_k, 0, max_dist) hits nothing with f itself skipped.  (front_open, front_total, back_open, back_total).

Fibonacci directions: z_i = 1 - (2 i + 1) / K, phi_i = pi (1 + sqrt 5) (i + 1/2), (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z)
in fp64, rounded to fp32.
"""
import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32


def valid_rays(o, d, tmin, tmax):
    o, d = np.asarray(o, F64), np.asarray(d, F64)
    tmin, tmax = np.asarray(tmin, F64), np.asarray(tmax, F64)
    with np.errstate(invalid='ignore'):
        return (np.isfinite(o).all(-1) & np.isfinite(d).all(-1) & (d != 0).any(-1) & np.isfinite(tmin) & ~np.isnan(tmax)
                & ~(tmax < tmin))


def shear(d):
    """(kx, ky, kz [n] integers, Sx, Sy, Sz [n] fp64) of directions d [n, 3] fp64, none of them 0"""
    kz = np.argmax(np.abs(d), axis=1)                       # the first maximum: the lowest axis among equals
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    r = np.arange(len(d))
    swap = d[r, kz] < 0.0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    dz = d[r, kz]
    return kx, ky, kz, d[r, kx] / dz, d[r, ky] / dz, 1.0 / dz


def edge_functions(o, d, verts, faces):
    """(U, V, W, det, tnum) [n, F] fp64 of valid rays (o, d) [n, 3] fp64: t = tnum / det"""
    kx, ky, kz, Sx, Sy, Sz = shear(d)
    A = verts.astype(F64)[None, :, :] - o[:, None, :]         # [n, V, 3]
    pick = lambda k: np.take_along_axis(A, np.broadcast_to(k[:, None, None], A.shape[:2] + (1,)), 2)[..., 0]
    Ax, Ay, Az = pick(kx), pick(ky), pick(kz)
    Px = Ax - Sx[:, None] * Az                                  # [n, V]
    Py = Ay - Sy[:, None] * Az
    Pz = Sz[:, None] * Az
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    U = Px[:, c] * Py[:, b] - Py[:, c] * Px[:, b]
    V = Px[:, a] * Py[:, c] - Py[:, a] * Px[:, c]
    W = Px[:, b] * Py[:, a] - Py[:, b] * Px[:, a]
    det = (U + V) + W
    tnum = (U * Pz[:, a] + V * Pz[:, b]) + W * Pz[:, c]
    return U, V, W, det, tnum


def cast_rays(o, d, tmin, tmax, verts, faces, skip=None, chunk=1 << 19):
    """(face [N] int32, t [N] fp32, bary [N, 2] fp32, t64 [N] fp64) by brute force, `chunk` ray-vertex pairs at a time.  o may be
    fp32 or fp64; tmin / tmax scalars or [N]."""
    o, d = np.asarray(o), np.asarray(d)
    N = len(o)
    faces = np.asarray(faces).astype(np.int64)
    tmin = np.broadcast_to(np.asarray(tmin, F32), (N,)).astype(F64)
    tmax = np.broadcast_to(np.asarray(tmax, F32), (N,)).astype(F64)
    skip = np.full(N, -1, np.int64) if skip is None else np.asarray(skip).astype(np.int64)
    ok = valid_rays(o, d, tmin, tmax)
    face = np.full(N, -1, I32)
    t64 = np.where(ok, np.inf, np.nan)
    bary = np.full((N, 2), np.nan, F32)
    idx = np.nonzero(ok)[0]
    step = max(1, chunk // max(len(verts), len(faces), 1))
    fid = np.arange(len(faces))
    for s in range(0, len(idx), step):
        i = idx[s:s + step]
        U, V, W, det, tnum = edge_functions(o[i].astype(F64), d[i].astype(F64), verts, faces)
        cand = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
        cand &= det != 0
        cand &= fid[None, :] != skip[i][:, None]
        with np.errstate(divide='ignore', invalid='ignore'):
            t = tnum / det
            hit = cand & (t >= tmin[i][:, None]) & (t <= tmax[i][:, None])
            t = np.where(hit, t, np.inf)
            f = np.argmin(t, axis=1)                            # the first minimum: the lowest face index among equals
            r = np.arange(len(i))
            any_hit = hit[r, f]
            face[i] = np.where(any_hit, f, -1)
            t64[i] = np.where(any_hit, t[r, f], np.inf)
            bv, bw = V[r, f] / det[r, f], W[r, f] / det[r, f]
        bary[i, 0] = np.where(any_hit, bv, np.nan).astype(F32)
        bary[i, 1] = np.where(any_hit, bw, np.nan).astype(F32)
    with np.errstate(over='ignore'):
        return face, t64.astype(F32), bary, t64


def moller_trumbore_hits(o, d, verts, faces):
    """[N] bool: does the plain fp64 Moller-Trumbore test (0 <= u, 0 <= v, u + v <= 1, t >= 0) find a hit -- the naive test the
    watertight one is compared with"""
    o, d = np.asarray(o, F64), np.asarray(d, F64)
    tri = verts.astype(F64)[np.asarray(faces)]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    out = np.zeros(len(o), bool)
    for n in range(len(o)):
        p = np.cross(d[n], e2)
        det = (e1 * p).sum(1)
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = 1.0 / det
            s = o[n] - a
            u = (s * p).sum(1) * inv
            q = np.cross(s, e1)
            v = (q * d[n]).sum(1) * inv
            t = (q * e2).sum(1) * inv
            out[n] = np.any((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0))
    return out


def fibonacci_directions(K):
    i = np.arange(K, dtype=F64)
    z = 1.0 - (2.0 * i + 1.0) / K
    phi = np.pi * (1.0 + np.sqrt(5.0)) * (i + 0.5)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(F32)


def face_openness(verts, faces, directions, max_dist=np.inf, chunk=1 << 19):
    """(front_open, front_total, back_open, back_total) int32 [F]"""
    v = verts.astype(F64)
    faces = np.asarray(faces).astype(np.int64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    cen = ((a + b) + c) / 3.0
    u, w = b - a, c - a
    N = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                  u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    F = len(faces)
    out = np.zeros((4, F), I32)
    me = np.arange(F)
    for dk in np.asarray(directions, F32):
        dd = dk.astype(F64)
        nd = (N[:, 0] * dd[0] + N[:, 1] * dd[1]) + N[:, 2] * dd[2]
        face = cast_rays(cen, np.broadcast_to(dk, (F, 3)), 0.0, max_dist, verts, faces, skip=me, chunk=chunk)[0]
        is_open = face < 0
        out[0] += (nd > 0) & is_open
        out[1] += nd > 0
        out[2] += (nd < 0) & is_open
        out[3] += nd < 0
    return tuple(out)


# ---- meshes for the tests ---------------------------------------------------------------------------------------------

def icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(verts fp32, faces int32) of the icosahedron subdivided `level` times (20 4^level faces), outward oriented, vertices
    normalised in fp64 and rounded to fp32; shared vertices are shared"""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, F64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.asarray(v, F64) * radius + np.asarray(center, F64)).astype(F32)
    return verts, np.asarray(f, I32)


def nested_spheres(level=2):
    """an icosphere at radius 1 plus its copy at radius 0.5, both outward oriented: (verts, faces, n_outer_faces)"""
    v1, f1 = icosphere(level, 1.0)
    v2, f2 = icosphere(level, 0.5)
    return np.concatenate([v1, v2]), np.concatenate([f1, f2 + len(v1)]).astype(I32), len(f1)


def lattice_mesh():
    """64 faces with vertices on integer planes of the box [0, 4]^3 and faces lying IN cell planes of a 4^3 (or 8 x 8 x 4, 16^3)
    grid: 8 unit quads (two triangles each) in each of the planes x = 2, y = 1, z = 3, z = 0, so that every grid of the tests has
    faces on its cell planes"""
    verts, faces = [], []

    def quad(p, e1, e2):
        n = len(verts)
        p, e1, e2 = (np.asarray(x, F64) for x in (p, e1, e2))
        verts.extend([p, p + e1, p + e1 + e2, p + e2])
        faces.extend([(n, n + 1, n + 2), (n, n + 2, n + 3)])
    cells = [(0, 0), (1, 1), (2, 3), (3, 0), (0, 2), (3, 3), (1, 2), (2, 1)]
    for i, j in cells:
        quad((2, i, j), (0, 1, 0), (0, 0, 1))
        quad((i, 1, j), (1, 0, 0), (0, 0, 1))
        quad((i, j, 3), (1, 0, 0), (0, 1, 0))
        quad((i, j, 0), (1, 0, 0), (0, 1, 0))
    return np.asarray(verts, F32), np.asarray(faces, I32)


def lattice_rays(seed=0):
    """(o, d, tmin, tmax) fp32 for lattice_mesh(): rays that run inside cell planes, along the diagonals, axis-parallel through
    lattice points, random ones, and tmin / tmax cuts of all of them"""
    rng = np.random.default_rng(seed)
    o, d = [], []
    for a in range(3):                                           # inside the plane x_a = p: origin on it, direction within it
        for p in (0.0, 1.0, 2.0, 3.0, 4.0):
            oo = rng.uniform(-1, 5, (12, 3))
            dd = rng.standard_normal((12, 3))
            oo[:, a], dd[:, a] = p, 0.0
            oo[:6] = np.round(oo[:6] * 2) / 2                     # half of them through lattice and half-lattice points
            dd[:3] = np.round(dd[:3])
            dd[np.all(dd == 0, 1)] = np.roll(np.eye(3)[a], 1)
            o.append(oo)
            d.append(dd)
    diag = np.asarray([[1, 1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, -1], [-1, -1, -1], [1, 1, 0], [0, 1, -1], [-1, 0, 1]], F64)
    for s in diag:
        for start in ((0, 0, 0), (4, 4, 4), (2, 1, 3), (0.5, 0.5, 0.5), (-1, -1, -1), (2, 2, 2), (1, 3, 0), (0, 4, 2)):
            o.append(np.asarray([start], F64) - 0.0 * s)
            d.append(s[None])
    for a in range(3):                                           # axis-parallel through lattice points, from outside and inside
        for sign in (1.0, -1.0):
            oo = np.round(rng.uniform(0, 4, (24, 3)) * 2) / 2
            oo[:12, a] = -2.0 if sign > 0 else 6.0
            dd = np.zeros((24, 3))
            dd[:, a] = sign
            o.append(oo)
            d.append(dd)
    n_rand = 270
    oo = rng.uniform(-2, 6, (n_rand, 3))
    oo[:150] = rng.uniform(0, 4, (150, 3))
    dd = rng.standard_normal((n_rand, 3))
    o.append(oo)
    d.append(dd)
    o, d = np.concatenate(o).astype(F32), np.concatenate(d).astype(F32)
    n = len(o)
    tmin, tmax = np.zeros(n, F32), np.full(n, np.inf, F32)
    # the same rays cut: tmax below, at and above lattice distances; tmin beyond the first hit
    cuts = [(0.0, 1.0), (0.0, 2.5), (1.0, 3.0), (2.0, np.inf), (0.5, 0.5)]
    os_, ds_, lo_, hi_ = [o], [d], [tmin], [tmax]
    for k, (lo, hi) in enumerate(cuts):
        pick = np.arange(k, n, len(cuts))
        os_.append(o[pick])
        ds_.append(d[pick])
        lo_.append(np.full(len(pick), lo, F32))
        hi_.append(np.full(len(pick), hi, F32))
    return np.concatenate(os_), np.concatenate(ds_), np.concatenate(lo_), np.concatenate(hi_)
