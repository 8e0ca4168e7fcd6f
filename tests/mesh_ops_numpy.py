"""numpy restatement of the mesh clean-up (csrc/mesh_ops.hip; ops.mesh_corner_table / mesh_vertex_normals / mesh_smooth /
mesh_cluster), written from the definitions alone -- the role tests/components_numpy.py has for the components.

verts [V, 3] fp32, faces [F, 3] integers, counter-clockwise seen from outside.  Corner c = 3 f + k is vertex faces[f, k].

Lists: for keys [n] in [0, K), offsets [K + 1] and items [n] with items[offsets[k]:offsets[k + 1]] = the i with keys[i] == k,
ascending (a stable sort of the keys).  keys = faces.reshape(-1), K = V: the corner table.  Every sum below runs over one
list front to back in fp64.

Normals: sum over the vertex's corners c of (p1 - p0) x (p2 - p0), p0 p1 p2 the vertices of face c // 3 in the face's own
order; divided by sqrt(n . n) per component; (0, 0, 0) for an empty list or a sum that is not > 0.  rounding='fp32' rounds
the result to fp32 (the kernel's one rounding point), 'fp64' leaves it.

Smoothing pass of weight w: s = sum over v's corners of (a + b), a = faces[f, (k + 1) % 3], b = faces[f, (k + 2) % 3];
out = v + w (s / (2 n) - v); n == 0: out = v.  Taubin: passes lam, mu in turn.  rounding='fp32' rounds the positions to
fp32 after every pass (the kernel's rounding point), 'fp64' never.

Clustering: the bit grid with box origin `origin`, inv = fp32(1 / cell), counts floorf(fp32(max - origin) * inv) + 1; cell of
a vertex per axis floorf(fp32(fp32(p - origin) * inv)); cluster id = rank of the cell in linear order (z fastest).  Per
cluster, C = origin + (ijk + 0.5) * cell in fp64; mean m = (sum over members, ascending, of (p - C)) / n; quadric: over the
cluster's corner list, q_i = p_i - C of face c // 3, N = (q1 - q0) x (q2 - q0), d = -(N . q0), A += N N^T, B += d N; det by
the cofactors of the first row, x = -(cof . B) / det, taken iff |det| > 1e-6 (trace / 3)^3 and fp32(C + x) falls in the
cluster's own cell by the cell rule; else the mean.  Colours (2 sum + n) // (2 n).  Faces remapped; dropped with two equal
ids, with dedupe also when an earlier face has the same directed cycle up to rotation; kept in order; unreferenced clusters
dropped, the rest renumbered in order.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def lists(keys, n_lists):
    keys = np.asarray(keys, np.int64).reshape(-1)
    assert keys.size == 0 or (keys.min() >= 0 and keys.max() < n_lists)
    items = np.argsort(keys, kind='stable').astype(np.int32)
    offsets = np.zeros(n_lists + 1, np.int64)
    np.cumsum(np.bincount(keys, minlength=n_lists), out=offsets[1:])
    return offsets.astype(np.int32), items


def corner_table(faces, n_verts):
    return lists(np.asarray(faces).reshape(-1), n_verts)


def _ordered_sum(values, keys, n_lists):
    """out[k] = sum of values[i] over keys[i] == k, added one by one in ascending i (fp64), as a loop over the lists does."""
    offsets, items = lists(keys, n_lists)
    out = np.zeros((n_lists,) + values.shape[1:], F64)
    counts = np.diff(offsets)
    for step in range(int(counts.max()) if counts.size else 0):
        sel = np.nonzero(counts > step)[0]
        out[sel] = out[sel] + values[items[offsets[sel] + step]]
    return out


def _cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                     u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)


def vertex_normals(verts, faces, rounding='fp32'):
    p = np.asarray(verts, F32).astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = p.shape[0]
    fn = _cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])                  # [F, 3]
    s = _ordered_sum(np.repeat(fn, 3, axis=0), f.reshape(-1), V)                  # corner c carries the normal of face c // 3
    n2 = s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]
    ok = (n2 > 0) & np.isfinite(n2)
    out = np.zeros((V, 3), F64)
    out[ok] = s[ok] / np.sqrt(n2[ok])[:, None]
    return out.astype(F32) if rounding == 'fp32' else out


def smooth_pass(p, faces, w):
    """One pass on fp64 positions p [V, 3]; returns fp64."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = p.shape[0]
    a = p[np.roll(f, -1, axis=1).reshape(-1)]                                      # corner 3 f + k: faces[f, (k + 1) % 3]
    b = p[np.roll(f, -2, axis=1).reshape(-1)]
    s = _ordered_sum(a + b, f.reshape(-1), V)
    n = np.bincount(f.reshape(-1), minlength=V).astype(F64)
    out = p.copy()
    has = n > 0
    out[has] = p[has] + w * (s[has] / (2.0 * n[has])[:, None] - p[has])
    return out


def smooth(verts, faces, iters=10, lam=0.5, mu=-0.53, rounding='fp32'):
    p = np.asarray(verts, F32).astype(F64)
    for _ in range(iters):
        for w in (lam, mu):
            p = smooth_pass(p, faces, w)
            if rounding == 'fp32':
                p = p.astype(F32).astype(F64)
    return p.astype(F32) if rounding == 'fp32' else p


def cluster_grid(verts, cell, origin=None):
    v = np.asarray(verts, F32)
    o = v.min(0) if origin is None else np.asarray(origin, F32)
    inv = F32(1.0 / float(cell))
    cells = tuple(int(x) + 1 for x in np.floor((v.max(0) - o).astype(F32) * inv))
    return o, inv, cells


def cell_of(points, o, inv, cells):
    """linear cell of fp32 points [P, 3] by the bit grid's rule, -1 outside."""
    with np.errstate(invalid='ignore'):
        f = np.floor(((np.asarray(points, F32) - o).astype(F32) * inv).astype(F32))
        inside = np.all((f >= 0) & (f < np.asarray(cells, F32)), axis=1)
    f = np.where(inside[:, None], f, 0).astype(np.int64)
    return np.where(inside, (f[:, 0] * cells[1] + f[:, 1]) * cells[2] + f[:, 2], -1)


def canonical_cycles(faces):
    """each face rotated so that its lowest id comes first (faces with three different ids)."""
    f = np.asarray(faces, np.int64)
    k = np.argmin(f, axis=1)
    i = np.arange(len(f))
    return np.stack([f[i, k], f[i, (k + 1) % 3], f[i, (k + 2) % 3]], -1)


def cluster(verts, faces, colors, origin, cell, placement='quadric', dedupe=False):
    """-> dict(verts fp32 [V', 3], faces int32 [F', 3], colors uint8 [V', 3] | None, cluster_of_vertex int32 [V],
    cells, origin, inv, cell_of_cluster [V'] (linear cell of every output vertex), used_quadric [V'] bool,
    det_margin [V'] (| |det| / threshold - 1 |, inf where the threshold is 0), wall_margin [V'] (distance of the quadric
    minimiser from its cell's wall in units of cell, negative outside; inf where the determinant test failed))."""
    v32 = np.asarray(verts, F32)
    p = v32.astype(F64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(p)
    o, inv, cells = cluster_grid(v32, cell, origin)
    assert all(1 <= c <= 512 for c in cells)
    lin = cell_of(v32, o, inv, cells)
    assert np.all(lin >= 0), 'a vertex outside the box'
    occupied = np.unique(lin)                                                      # ascending linear cell = cluster id
    cov = np.searchsorted(occupied, lin)
    K = len(occupied)
    cell = float(cell)
    ijk = np.stack([occupied // (cells[1] * cells[2]), (occupied // cells[2]) % cells[1], occupied % cells[2]], -1)
    C = o.astype(F64) + (ijk.astype(F64) + 0.5) * cell
    n_mem = np.bincount(cov, minlength=K)
    mean = _ordered_sum(p - C[cov], cov, K) / n_mem[:, None].astype(F64)
    pos = mean.copy()
    used = np.zeros(K, bool)
    det_margin = np.full(K, np.inf)
    wall_margin = np.full(K, np.inf)
    rf = cov[f]
    if placement == 'quadric' and len(f):
        keys = rf.reshape(-1)                                                      # corner c belongs to cluster keys[c]
        Cc = C[keys]
        q0, q1, q2 = (np.repeat(p[f[:, t]], 3, axis=0) - Cc for t in range(3))     # face c // 3 relative to the corner's cluster
        N = _cross(q1 - q0, q2 - q0)
        d = -(N[:, 0] * q0[:, 0] + N[:, 1] * q0[:, 1] + N[:, 2] * q0[:, 2])
        terms = np.stack([N[:, 0] * N[:, 0], N[:, 0] * N[:, 1], N[:, 0] * N[:, 2], N[:, 1] * N[:, 1], N[:, 1] * N[:, 2],
                          N[:, 2] * N[:, 2], d * N[:, 0], d * N[:, 1], d * N[:, 2]], -1)
        S = _ordered_sum(terms, keys, K)
        a00, a01, a02, a11, a12, a22, b0, b1, b2 = (S[:, t] for t in range(9))
        t3 = (a00 + a11 + a22) / 3.0
        thr = 1e-6 * (t3 * t3 * t3)
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = a00 * c00 + a01 * c01 + a02 * c02
        good = np.abs(det) > thr
        with np.errstate(divide='ignore', invalid='ignore'):
            det_margin = np.where(thr > 0, np.abs(np.abs(det) / thr - 1.0), np.inf)
            x = np.stack([-(c00 * b0 + c01 * b1 + c02 * b2) / det, -(c01 * b0 + c11 * b1 + c12 * b2) / det,
                          -(c02 * b0 + c12 * b1 + c22 * b2) / det], -1)
        x = np.where(good[:, None], x, 0.0)
        inside = cell_of((C + x).astype(F32), o, inv, cells) == occupied
        wall_margin = np.where(good, (0.5 * cell - np.abs(x).max(1)) / cell, np.inf)
        used = good & inside
        pos[used] = x[used]
    rep = (C + pos).astype(F32)
    rep_colors = None
    if colors is not None:
        col = np.asarray(colors, np.uint8).astype(np.int64)
        sums = np.stack([np.bincount(cov, weights=col[:, t], minlength=K) for t in range(3)], -1).astype(np.int64)
        rep_colors = ((2 * sums + n_mem[:, None]) // (2 * n_mem[:, None])).astype(np.uint8)
    keep = (rf[:, 0] != rf[:, 1]) & (rf[:, 1] != rf[:, 2]) & (rf[:, 0] != rf[:, 2]) if len(f) else np.zeros(0, bool)
    if dedupe and keep.any():
        idx = np.nonzero(keep)[0]
        _, first = np.unique(canonical_cycles(rf[idx]), axis=0, return_index=True)
        keep = np.zeros(len(f), bool)
        keep[idx[first]] = True
    kept = rf[keep]
    referenced = np.zeros(K, bool)
    referenced[kept.reshape(-1)] = True
    new_id = np.cumsum(referenced) - 1
    return dict(verts=rep[referenced], faces=new_id[kept].astype(np.int32).reshape(-1, 3),
                colors=None if rep_colors is None else rep_colors[referenced],
                cluster_of_vertex=np.where(referenced[cov], new_id[cov], -1).astype(np.int32), cells=cells, origin=o, inv=inv,
                cell_of_cluster=occupied[referenced], used_quadric=used[referenced], det_margin=det_margin[referenced],
                wall_margin=wall_margin[referenced])


# ---- the analytic lattices the tests mesh (marching cubes: mesh.marching_cubes on the GPU, tests/mc_numpy.py on the CPU) -----
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def lattice(n, fn):
    ax = [F32(LO[a]) + np.arange(n, dtype=F32) * ((F32(HI[a]) - F32(LO[a])) / F32(n - 1)) for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing='ij')
    return np.ascontiguousarray(fn(x, y, z), dtype=F32)


def sphere_field(r=0.6, c=(0.0, 0.0, 0.0)):
    return lambda x, y, z: 2.0 - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / r


def two_spheres_field(x, y, z):
    return np.maximum(sphere_field(0.35, (-0.45, -0.1, 0.05))(x, y, z), sphere_field(0.3, (0.5, 0.15, -0.1))(x, y, z))


def torus_field(x, y, z, R=0.55, r=0.25):
    return 2.0 - np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) / r


def step(n):
    """the lattice step of an n^3 lattice on [LO, HI]."""
    return 2.0 / (n - 1)


# (name, lattice points per axis, field, cell in lattice steps, origin: None = the vertices' minimum, 'box' = LO).  The iso value
# is 1 throughout.  'box' with an even number of steps puts mesh vertices exactly on cell faces (the floorf rule); the torus at 6
# steps has clusters of more than 64 corners.
CLUSTER_CASES = (
    ('sphere24_3', 24, sphere_field(), 3.0, None),
    ('sphere24_2box', 24, sphere_field(0.6, (0.07, -0.04, 0.11)), 2.0, 'box'),
    ('two_spheres24_2.5', 24, two_spheres_field, 2.5, None),
    ('torus32_6', 32, torus_field, 6.0, None),
)
# The cases whose quadric positions are compared, under the cap on borderline clusters.  Not sphere24_2box: three quarters of
# its vertices lie exactly on cell faces, so some clusters have all their members in one wall plane and their planes meet ON the
# wall (9 % of the clusters have a minimiser within 1e-6 cell of it).  It is there for the floorf rule: its integers are
# compared under both placements and its positions bit for bit under 'mean'.
QUADRIC_CASES = ('sphere24_3', 'two_spheres24_2.5', 'torus32_6')
# a cluster whose quadric decision lies this close to one of its two thresholds is left out of the position comparison
DET_MARGIN, WALL_MARGIN = 1e-3, 1e-3
MAX_SKIPPED_SHARE = 0.01


def borderline(res):
    """clusters of a quadric cluster() result that the GPU comparison leaves out."""
    return (res['det_margin'] < DET_MARGIN) | (np.abs(res['wall_margin']) < WALL_MARGIN)


# ---- first-principles helpers for the tests --------------------------------------------------------------------------------
def directed_edge_balance(faces):
    """max over directed edges (a, b), a != b, of | count(a, b) - count(b, a) |: 0 for a closed, consistently oriented mesh."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return 0
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e = e[e[:, 0] != e[:, 1]]
    n = int(f.max()) + 1
    fwd = dict(zip(*np.unique(e[:, 0] * n + e[:, 1], return_counts=True)))
    return max(abs(c - fwd.get((k % n) * n + k // n, 0)) for k, c in fwd.items())
